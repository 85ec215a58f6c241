"""The spectrum whitening on the GPU (``pss_spectrum_medians``,
``pss_spectrum_whiten``, ``Backend.spectrum_medians`` / ``whiten_spectrum`` and
the ``whiten=`` / ``zap=`` keywords of the spectral searches).

The oracle is tests/whiten_ref.py: a sort of the uint32 keys for the medians,
NumPy float32 with one rounded operation per line for the rest.  A selection is
exact and the arithmetic is fixed, so every comparison is ``array_equal`` on
the uint32 view -- no tolerance, no excluded bin.

Every kernel-level case gives the kernels views inside larger tensors
(tests/kernel_harness.py): the spectrum with a row stride ld > nbin between
guards of 2^20, the outputs inside a sentinel that is checked untouched
afterwards -- in place, the columns [nbin, ld) of the spectrum itself.

The kernels' tiles (pss_whiten.hip): a wave selects from one block, by its
width with 1, 2 or 4 keys a lane (the widths 64 / 65 and 128 / 129 are the
thresholds), a workgroup owns 32 consecutive blocks; the whitening owns 1024
bins a workgroup and moves 16, 8 or 4 bytes a lane by the alignment.
"""
import numpy as np
import pytest

from tests import periodicity_ref as pref
from tests import whiten_ref as ref
from tests import kernel_harness as kh
from tests.kernel_harness import same_bits

pytestmark = pytest.mark.gpu

IN_GUARD = float(1 << 20)
OUT_GUARD = -7.0
HAND = [1, 256, 2, 255, 3, 64, 65, 128]


def noise(ndm, nbin, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((ndm, nbin, 2)).astype(np.float32)
    x *= np.geomspace(30.0, 1.0, nbin, dtype=np.float32)[None, :, None]       # a red spectrum
    return np.ascontiguousarray(x).view(np.complex64)[..., 0]


def spoil(x, edges, most_inf):
    """The last trial's blocks 1 .. get, in turn: repeated powers (ties), all
    zeros, one NaN, NaN in half the bins and one more (a NaN median), one +inf
    and -- ``most_inf`` -- +inf in most bins (an infinite median)."""
    x = x.copy()
    row = x[-1]
    nblk = len(edges) - 1
    roles = ["ties", "zeros", "nan1", "nanhalf", "inf1"] + (["infmost"] if most_inf else [])
    for i, role in enumerate(roles):
        b = i + 1
        if b >= nblk:
            break
        lo, hi = int(edges[b]), int(edges[b + 1])
        w = hi - lo
        if role == "ties":
            row[lo:hi] = (np.round(row[lo:hi].real) + 1j * np.round(row[lo:hi].imag)).astype(np.complex64)
        elif role == "zeros":
            row[lo:hi] = 0
        elif role == "nan1":
            row[lo + w // 3] = complex(np.nan, 0.0)
        elif role == "nanhalf":
            row[lo:lo + w // 2 + 1] = complex(0.5, np.nan)
        elif role == "inf1":
            row[lo + w // 2] = complex(np.inf, 1.0)
        else:
            row[lo:lo + (3 * w) // 4 + 1] = complex(1.0, -np.inf)
    return x


def table(widths, e0):
    return np.concatenate([[e0], e0 + np.cumsum(widths)]).astype(np.int64)


@kh.once
def case(name, ndm, most_inf):
    """(x complex64 [ndm][nbin], edges, med) of a named input: ``plan<nbin>``
    (the default plan; from bin 0 where nbin = 1; 1 and 7 bins give one block,
    13 bins two), ``hand<e0>``, ``two<e0>`` (two blocks) and ``w256``."""
    if name.startswith("plan"):
        nbin = int(name[4:])
        edges = ref.plan_ref(nbin, kstart=min(1, nbin - 1))
    elif name.startswith("hand"):
        edges = table(HAND, int(name[4:]))
    elif name.startswith("two"):
        edges = table([5, 9], int(name[3:]))                       # two blocks: one pair of centres, flat outside
    else:
        edges = table([256] * 9, 0)
    nbin = int(edges[-1])
    x = spoil(noise(ndm, nbin, 7 + ndm), edges, most_inf)
    return x, edges, ref.medians_ref(x, edges)


@kh.once
def whitened(name, ndm, with_zap):
    x, edges, med = case(name, ndm, False)
    nbin = x.shape[1]
    zap = None
    if with_zap:
        # runs at both ends of a block and across a block boundary (where there are such blocks)
        zap = np.zeros(nbin, dtype=np.uint8)
        b = min(2, len(edges) - 2)
        lo, hi = int(edges[b]), int(edges[b + 1])
        zap[lo:lo + 2] = 1
        zap[max(hi - 2, 0):hi] = 7
        if len(edges) > 4:
            zap[int(edges[3]) - 3:int(edges[3]) + 3] = 1
        zap[0] = 1                                             # below edges[0] in some cases: (0, 0) wins
        zap[nbin - 1] = 255
    return x, edges, med, zap, ref.whiten_ref(x, edges, med, zap)


def _spec_input(x, ld, in_off):
    return kh.GuardedInput(np.ascontiguousarray(x).view(np.float32).reshape(x.shape[0], x.shape[1], 2), ld, in_off,
                           IN_GUARD)


def run_medians(hip_lib, x, edges, ld=None, out_ld=None, in_off=0, out_off=0):
    import torch
    from psrsigsim_amd import _lib
    ndm, nbin = x.shape
    nblk = len(edges) - 1
    ld = nbin + 3 if ld is None else ld
    out_ld = nblk + 5 if out_ld is None else out_ld
    spec = _spec_input(x, ld, in_off)
    med = kh.GuardedOutput(ndm, nblk, out_ld, out_off, OUT_GUARD)
    e_d = torch.from_numpy(np.array(edges, dtype=np.int64)).cuda()
    torch.cuda.synchronize()
    rc = hip_lib.pss_spectrum_medians(spec.ptr, ndm, nbin, ld, e_d.data_ptr(), nblk, med.ptr, out_ld, None)
    _lib.check(rc, "spectrum_medians")
    torch.cuda.synchronize()
    return med.read()


def run_whiten(hip_lib, x, edges, med, zap, inplace, ld=None, out_ld=None, in_off=0, out_off=0):
    """pss_spectrum_whiten; returns out complex64 [ndm][nbin] after checking
    that nothing else was written: out of place the output's sentinel and the
    input as a whole, in place everything of the input's parent but the bins."""
    import torch
    from psrsigsim_amd import _lib
    ndm, nbin = x.shape
    nblk = len(edges) - 1
    ld = nbin + 3 if ld is None else ld
    out_ld = nbin + 2 if out_ld is None else out_ld
    spec = _spec_input(x, ld, in_off)
    before = spec.parent.cpu().numpy()
    e_d = torch.from_numpy(np.array(edges, dtype=np.int64)).cuda()
    m_d = torch.from_numpy(np.array(med, dtype=np.float32)).cuda()
    z_d = None if zap is None else torch.from_numpy(np.array(zap, dtype=np.uint8)).cuda()
    out = None if inplace else kh.GuardedOutput(ndm, 2 * nbin, 2 * out_ld, out_off, OUT_GUARD)
    torch.cuda.synchronize()
    rc = hip_lib.pss_spectrum_whiten(spec.ptr, ndm, nbin, ld, e_d.data_ptr(), nblk, m_d.data_ptr(), nblk,
                                     None if z_d is None else z_d.data_ptr(), spec.ptr if inplace else out.ptr,
                                     ld if inplace else out_ld, None)
    _lib.check(rc, "spectrum_whiten")
    torch.cuda.synchronize()
    after = spec.parent.cpu().numpy()
    if not inplace:
        assert before.tobytes() == after.tobytes(), "the input was written"
        got = out.read()
    else:
        lead = spec.view.data_ptr() // 4 - spec.parent.data_ptr() // 4
        body = np.zeros(after.size, dtype=bool)
        body[lead:lead + ndm * ld * 2].reshape(ndm, ld * 2)[:, :2 * nbin] = True
        assert before[~body].tobytes() == after[~body].tobytes(), "written outside the bins of a row"
        got = after[body].reshape(ndm, 2 * nbin)
    return np.ascontiguousarray(got).view(np.complex64)


CASES = ["plan1", "plan7", "plan13", "plan300", "plan2049", "plan4097", "two0", "two1", "two5", "hand0", "hand1",
         "hand5", "w256"]


# ---------------------------------------------------------------------------
# the medians
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ndm", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_medians_are_the_sorted_keys(hip_lib, name, ndm):
    x, edges, med = case(name, ndm, True)
    got = run_medians(hip_lib, x, edges)
    assert same_bits(got, med)
    if name == "w256":
        bits = got.view(np.uint32)[-1]
        assert bits[2] == 0 and bits[4] == 0x7FC00000 and bits[6] == 0x7F800000      # zeros, NaN, +inf


@pytest.mark.parametrize("name", ["plan2049", "hand5"])
def test_medians_alignment_and_pitch_do_not_matter(hip_lib, name):
    x, edges, med = case(name, 3, True)
    nbin, nblk = x.shape[1], len(edges) - 1
    odd = kh.odd
    for kw in list(kh.misaligned_layouts(nbin + 2 + nbin % 2, nblk + 4 - nblk % 4 + 4, odd(nbin + 2), odd(nblk + 2),
                                         in_off=2)) + [dict(ld=odd(nbin + 2), out_ld=nblk + 1, in_off=1, out_off=0),
                                                       dict(ld=nbin + 4, out_ld=odd(nblk + 2), in_off=3, out_off=1)]:
        assert same_bits(run_medians(hip_lib, x, edges, **kw), med), kw


# ---------------------------------------------------------------------------
# the whitening
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("with_zap", [False, True])
@pytest.mark.parametrize("ndm", [1, 3])
@pytest.mark.parametrize("name", CASES)
def test_whitening_is_the_restatement_in_place_and_out_of_place(hip_lib, name, ndm, with_zap):
    x, edges, med, zap, want = whitened(name, ndm, with_zap)
    out = run_whiten(hip_lib, x, edges, med, zap, False)
    assert same_bits(out.view(np.float32), want.view(np.float32))
    inp = run_whiten(hip_lib, x, edges, med, zap, True)
    assert same_bits(inp.view(np.float32), out.view(np.float32))
    again = run_whiten(hip_lib, x, edges, med, zap, True)
    assert same_bits(again.view(np.float32), inp.view(np.float32))                   # from run to run
    e0 = int(edges[0])
    assert not out[:, :e0].view(np.float32).any()
    if with_zap:
        z = np.flatnonzero(zap[e0:]) + e0
        assert z.size and np.all(out[:, z] == 1)


@pytest.mark.parametrize("name", ["plan2049", "plan4097", "hand1"])
def test_whitening_alignment_and_pitch_do_not_matter(hip_lib, name):
    """Every route of the launcher: 16-B accesses with rows on and off the
    16-B grid, 8-B accesses, dwords; spec and out aligned alike and not."""
    x, edges, med, zap, want = whitened(name, 3, True)
    nbin = x.shape[1]
    even = nbin + 2 + nbin % 2
    w32 = want.view(np.float32)
    for kw in (dict(ld=even, out_ld=even), dict(ld=even + 1, out_ld=even + 1), dict(ld=even + 1, out_ld=even + 3),
               dict(ld=even, out_ld=even + 1), dict(ld=even, out_ld=even, in_off=2), dict(ld=even, out_ld=even, out_off=2),
               dict(ld=even + 1, out_ld=even, in_off=2, out_off=2), dict(ld=even, out_ld=even, in_off=1),
               dict(ld=even + 1, out_ld=even + 1, out_off=1), dict(ld=even, out_ld=even, in_off=3, out_off=3)):
        assert same_bits(run_whiten(hip_lib, x, edges, med, zap, False, **kw).view(np.float32), w32), kw
    for kw in (dict(ld=even), dict(ld=even + 1), dict(ld=even, in_off=2), dict(ld=even + 1, in_off=2),
               dict(ld=even, in_off=1), dict(ld=even + 1, in_off=3)):
        assert same_bits(run_whiten(hip_lib, x, edges, med, zap, True, **kw).view(np.float32), w32), kw


def test_block_counts_of_the_cases():
    """nblk in {1, 2, many} is what the cases above hold."""
    n = {name: len(case(name, 1, False)[1]) - 1 for name in CASES}
    assert n["plan1"] == n["plan7"] == 1 and n["plan13"] == n["two0"] == n["two1"] == n["two5"] == 2
    assert n["hand0"] == 8 and n["w256"] == 9 and min(n["plan300"], n["plan2049"], n["plan4097"]) > 9


@pytest.mark.parametrize("name", ["two1", "hand1", "plan2049"])
def test_whitening_with_an_infinite_median(hip_lib, name):
    """norm = +inf gives s = 0, like a zero or a NaN median: a block's median
    set to +inf (and the last block's) over the finite bins of the case, so
    that its bins and those that interpolate towards it come out as re 0, im 0
    with the sign of the input.  (The medians' own infinite case is in
    test_medians_are_the_sorted_keys; its spectrum holds inf 0 products, whose
    NaN has no sign that IEEE fixes, so it is not compared here.)"""
    x, edges, med = case(name, 3, False)
    nblk = len(edges) - 1
    m = np.array(med)
    b = min(8, nblk - 1)                                          # (finite bins in it and in its neighbours)
    m[:, b] = np.inf
    m[1, nblk - 1] = np.inf
    want = ref.whiten_ref(x, edges, m)
    blk = np.ascontiguousarray(want[:, int(edges[b]):int(edges[b + 1])]).view(np.float32)
    assert not (blk != 0).any()                                   # +-0 throughout, no NaN
    out = run_whiten(hip_lib, x, edges, m, None, False)
    assert same_bits(out.view(np.float32), want.view(np.float32))
    assert same_bits(run_whiten(hip_lib, x, edges, m, None, True).view(np.float32), want.view(np.float32))


def test_the_two_kernels_in_a_row(hip_lib):
    """The device's medians into the device's whitening: the restatement's bits."""
    x, edges, med, zap, want = whitened("plan4097", 3, False)
    got = run_medians(hip_lib, x, edges)
    assert same_bits(got, med)
    assert same_bits(run_whiten(hip_lib, x, edges, got, None, True).view(np.float32), want.view(np.float32))


# ---------------------------------------------------------------------------
# the API
# ---------------------------------------------------------------------------
def _plane(x, samprate=0.01):
    import torch
    from psrsigsim_amd.telescope import DedispersedPlane
    x = np.asarray(x, dtype=np.float32)
    return DedispersedPlane(torch.from_numpy(np.array(x)).cuda(), np.arange(float(x.shape[0])),
                            np.zeros((x.shape[0], 1), dtype=np.int32), samprate, 1500.0, 0)


T_RED = 1 << 15
P_RED = 53.7
TONE = 1200


@kh.once
def red_series(tone):
    """4 trials x 2^15 samples: unit white noise plus 0.05 cumsum(white), a
    pulse of 3 samples and amplitude 0.9 every 53.7 samples in trial 2; with
    ``tone`` a line of amplitude 0.5 at bin 1200 and at its harmonics 2 and 3
    in every trial."""
    rng = np.random.default_rng(2)
    x = rng.standard_normal((4, T_RED))
    x = x + 0.05 * np.cumsum(rng.standard_normal((4, T_RED)), axis=1)
    t0 = np.floor(np.arange(int(T_RED / P_RED) + 1) * P_RED).astype(np.int64)
    for d in range(3):
        t = t0 + d
        x[2, t[t < T_RED]] += 0.9
    if tone:
        tt = np.arange(T_RED)
        for h in (1, 2, 3):
            x += 0.5 * np.cos(2 * np.pi * TONE * h * tt / T_RED)
    return x.astype(np.float32)


def _small():
    rng = np.random.default_rng(5)
    T = 4500
    x = rng.standard_normal((3, T)) + 0.1 * np.cumsum(rng.standard_normal((3, T)), axis=1)
    return x.astype(np.float32)


def test_api_medians_and_whitening(hip_lib):
    import torch
    from psrsigsim_amd.telescope import Backend
    be = kh.backend()
    plane = _plane(_small())
    spec = be.dm_spectrum(plane)
    nbin = int(spec.shape[1]) - 1
    host = spec.cpu().numpy()
    keep = host.copy()
    for plan in (None, Backend.whiten_plan(nbin, kstart=3, w0=2, wmax=17)):
        edges = ref.plan_ref(nbin) if plan is None else plan.edges
        med = be.spectrum_medians(spec, plan)
        assert med.dtype == torch.float32 and tuple(med.shape) == (3, len(edges) - 1)
        assert same_bits(med.cpu().numpy(), ref.medians_ref(host[:, :nbin], edges))
        zap = Backend.zap_mask(2 * nbin, 0.01, [(100.0, 130.0)])
        assert zap.sum() > 3
        for z in (None, zap, torch.from_numpy(zap).cuda(), torch.from_numpy(zap.astype(bool)).cuda()):
            zh = None if z is None else zap
            want = ref.whiten_ref(host[:, :nbin], edges, zap=zh)
            out = be.whiten_spectrum(spec, plan, zap=z)
            assert out.dtype == torch.complex64 and out.shape == spec.shape and out.data_ptr() != spec.data_ptr()
            o = out.cpu().numpy()
            assert same_bits(np.ascontiguousarray(o[:, :nbin]).view(np.float32), want.view(np.float32))
            assert o[:, nbin].tobytes() == host[:, nbin].tobytes()             # the Nyquist bin as it was
            assert spec.cpu().numpy().tobytes() == keep.tobytes()              # the caller's tensor is left alone
            work = spec.clone()
            same = be.whiten_spectrum(work, plan, zap=z, inplace=True)
            assert same.data_ptr() == work.data_ptr() and same.shape == work.shape
            assert same.cpu().numpy().tobytes() == o.tobytes()
    with pytest.raises(ValueError, match="in place"):
        be.whiten_spectrum(spec[:, ::2], inplace=True)


def test_search_on_red_noise(hip_lib):
    """Without whitening the search of red noise returns red noise: the
    strongest candidate sits below bin 16 and every trial has candidates
    (today's behaviour).  Whitened, the strongest is the pulsar of trial 2 at
    its 32768 / 53.7 = 610.2 bins, no pulsar-free trial has a cell at the
    threshold, and the maps are the restatement's on the device's own
    spectrum bit for bit.  On the CPU (NumPy's transform) the restatement gave
    [0, 0, 52, 0] cells a trial and a strongest cell at bin 9763, 16
    harmonics, z = 102.8; unwhitened [30, 24, 66, 29] and z = 1820 at bin 8."""
    import torch
    be = kh.backend()
    x = red_series(False)
    plane = _plane(x)
    df = 0.01 * 1e6 / T_RED
    kw = dict(threshold=12.0, fmin=8 * df)
    plain = be.periodicity_search(plane, **kw)
    assert plain.cells.kmin == 8 and plain.cells.whiten is None
    assert plain.freq[0] / df < 16
    assert set(plain.dm_index.tolist()) == {0, 1, 2, 3}
    white = be.periodicity_search(plane, whiten=True, **kw)
    cells = white.cells
    per_trial = (cells.snr >= 12.0).sum(dim=1).cpu().numpy()
    print("whitened: cells per trial %s, top snr %.2f bin %d nharm %d at %.4f bins; unwhitened top snr %.1f at %.2f bins"
          % (per_trial, white.snr[0], white.bin[0], white.nharm[0], white.freq[0] / df, plain.snr[0],
             plain.freq[0] / df))
    assert white.dm_index[0] == 2 and abs(white.freq[0] / df - T_RED / P_RED) <= 0.25
    assert per_trial[0] == 0 and per_trial[1] == 0 and per_trial[3] == 0 and per_trial[2] > 0
    assert np.array_equal(cells.whiten.edges, ref.plan_ref(T_RED // 2)) and cells.nbin == T_RED // 2
    # the restatement on the device's own spectrum (the FFT library's rounding is not ours)
    spec = be.dm_spectrum(plane)
    host = spec.cpu().numpy()
    nbin = T_RED // 2
    wref = ref.whiten_ref(host[:, :nbin], cells.whiten.edges)
    cands, snr, code = pref.search_ref(wref, 1.0, 12.0, 5, 8, 32)
    assert same_bits(cells.snr.cpu().numpy(), snr) and np.array_equal(cells.code.cpu().numpy(), code)
    assert np.array_equal((snr >= 12).sum(axis=1), per_trial)
    assert len(cands) == len(white) and cands[0][1:4] == (2, int(white.bin[0]), int(white.nharm[0]))
    assert np.float32(cands[0][0]) == white.snr[0]
    # std is reported as before but does not enter the normalisation
    assert torch.equal(cells.std, plain.cells.std) and torch.equal(cells.mean, plain.cells.mean)
    other = be.harmonic_snr(plane, whiten=True, fmin=8 * df, mean=cells.mean.cpu().numpy(),
                            std=7.0 * cells.std.cpu().numpy())
    assert same_bits(other.snr.cpu().numpy(), snr) and np.array_equal(other.code.cpu().numpy(), code)
    # a caller's spectrum is whitened out of place
    given = be.harmonic_snr(plane, whiten=True, fmin=8 * df, spectrum=spec)
    assert same_bits(given.snr.cpu().numpy(), snr) and np.array_equal(given.code.cpu().numpy(), code)
    assert spec.cpu().numpy().tobytes() == host.tobytes()
    # ... and one that has to be converted (here: not contiguous) is whitened in its converted copy
    wide = torch.zeros((4, int(spec.shape[1]) + 3), dtype=torch.complex64, device=spec.device)
    wide[:, :spec.shape[1]] = spec
    keep = wide.cpu().numpy().tobytes()
    view = wide[:, :spec.shape[1]]
    assert not view.is_contiguous()
    given = be.harmonic_snr(plane, whiten=True, fmin=8 * df, spectrum=view)
    assert same_bits(given.snr.cpu().numpy(), snr) and np.array_equal(given.code.cpu().numpy(), code)
    assert wide.cpu().numpy().tobytes() == keep
    # chunks of one trial: the same maps
    part = be.harmonic_snr(plane, whiten=True, fmin=8 * df, max_bytes=(nbin + 1) * 8)
    assert same_bits(part.snr.cpu().numpy(), snr) and np.array_equal(part.code.cpu().numpy(), code)


def test_zapping_removes_a_line(hip_lib):
    from psrsigsim_amd.telescope import Backend
    be = kh.backend()
    plane = _plane(red_series(True))
    df = 0.01 * 1e6 / T_RED
    kw = dict(threshold=12.0, fmin=8 * df, whiten=True)
    lined = be.harmonic_snr(plane, fmin=8 * df, whiten=True)
    top = lined.snr.argmax(dim=1, keepdim=True)
    fund = (lined.freq.gather(1, top)[:, 0] / df).cpu().numpy()
    print("with the line: top fundamentals %s bins, snr %s" % (fund, lined.snr.amax(dim=1).cpu().numpy()))
    assert np.all(np.abs(fund - TONE) <= 0.5)                      # the line, at every DM
    ranges = [(h * TONE * df - 0.25 * df, h * TONE * df + 0.25 * df) for h in (1, 2, 3)]
    mask = Backend.zap_mask(T_RED, 0.01, ranges)
    assert np.array_equal(np.flatnonzero(mask), [TONE, 2 * TONE, 3 * TONE])
    clean = be.periodicity_search(plane, zap=mask, **kw)
    bins = clean.freq / df
    print("zapped: top snr %.2f in trial %d at %.4f bins" % (clean.snr[0], clean.dm_index[0], bins[0]))
    assert clean.dm_index[0] == 2 and abs(bins[0] - T_RED / P_RED) <= 0.25
    for h in (0.5, 1, 2, 3):
        assert not np.any(np.abs(bins - h * TONE) <= 1.0)           # the line is gone
    assert set(clean.dm_index.tolist()) == {2}
    with pytest.raises(ValueError, match="zap needs whiten"):
        be.periodicity_search(plane, threshold=12.0, zap=mask)


def test_acceleration_search_whitens_too(hip_lib):
    import torch
    from psrsigsim_amd.telescope import Backend
    be = kh.backend()
    x = _small()
    T = x.shape[1]
    plane = _plane(x)
    zap = Backend.zap_mask(Backend.fft_length(T), 0.01, [(200.0, 210.0)])
    for kw in (dict(whiten=True), dict(whiten=dict(w0=3, wmax=40), zap=zap, nharm=4)):
        h = be.harmonic_snr(plane, **kw)
        a = be.accel_snr(plane, [0.0], **kw)
        assert torch.equal(a.snr.view(torch.int32), h.snr.view(torch.int32)) and torch.equal(a.code, h.code)
        assert np.array_equal(a.whiten.edges, h.whiten.edges)
    acc = [0.0, float(Backend.accel_trials(T, 0.01, 2.4e6, tol=1.0)[-1])]
    full = be.accel_snr(plane, acc, whiten=True)
    assert int(full.acc_index.max()) == 1
    nbin = Backend.fft_length(T) // 2
    per_row = T * 4 + (nbin + 1) * 8 + nbin * 4
    # 2 rows a chunk: one trial with both accelerations; 1 row: the accelerations of a trial split
    for mb in (2 * per_row + 100, per_row):
        part = be.accel_snr(plane, acc, whiten=True, max_bytes=mb)
        assert torch.equal(part.snr.view(torch.int32), full.snr.view(torch.int32))
        assert torch.equal(part.code, full.code) and torch.equal(part.acc_index, full.acc_index)
    c = be.accel_search(plane, accels=acc, whiten=True, threshold=8.0)
    assert c.cells.whiten is not None


def test_off_means_off(hip_lib):
    import torch
    be = kh.backend()
    plane = _plane(_small())
    a = be.harmonic_snr(plane)
    for kw in (dict(whiten=None), dict(whiten=False), dict(whiten=None, zap=None)):
        b = be.harmonic_snr(plane, **kw)
        assert b.whiten is None
        assert torch.equal(a.snr.view(torch.int32), b.snr.view(torch.int32)) and torch.equal(a.code, b.code)
    w = be.harmonic_snr(plane, whiten=True)
    assert not torch.equal(a.snr.view(torch.int32), w.snr.view(torch.int32))
