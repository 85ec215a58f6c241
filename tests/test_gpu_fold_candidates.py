"""The candidate fold on the GPU (``pss_fold_series``,
``Backend.fold_candidates``, ``FoldedCandidates.refine``).

The oracle is tests/fold_ref.py: the 64-bit fixed-point phase restated with
uint64 arrays and ``np.bincount`` in float64.  Index tests use integer-valued
float32 data (seeded integers 0 .. 15): every partial sum is an exact float32
in any order (15 L < 2^24) and the comparison is ``array_equal`` -- no
tolerance, no excluded element -- for the sums and for the hits, and every
(row, sub-integration) must hold exactly L hits.  Every kernel-level case gives
the kernel views inside larger tensors (row stride ld > T): the input's guard
rows and columns hold 2^20 (a read outside [0, nsub L) of the row the clamped
table names lands in a sum and breaks the equality -- the guards are at least
five rows wide on either side, so a table index that went unclamped would
still read allocated memory), the outputs' guards hold a sentinel and are
checked untouched afterwards.

The kernel (pss_foldseries.hip) stages a sub-integration in chunks of CH = 4096
samples; below 256 bins G = 256 // nbin threads share a bin, taking turns up to
a period of CH // G samples and splitting every run beyond.
"""
import numpy as np
import pytest

from tests import fold_ref as ref
from tests import kernel_harness as kh
from tests.kernel_harness import engine_seed_restored  # noqa: F401 (autouse here)

pytestmark = pytest.mark.gpu

CH = 4096                               # kFsChunk
IN_GUARD = float(1 << 20)
OUT_GUARD = -7.0
HIT_GUARD = -9
TWO64 = 1 << 64


def int_data(nser, T, seed):
    return np.random.default_rng(seed).integers(0, 16, size=(nser, T)).astype(np.float32)


def _case(name):
    """dict(x [nser][T] float32, src, inc, phi0 (Python ints), nsub, L, nbin)."""
    if name == "one":                                    # 1: alternate samples
        return dict(x=int_data(1, 64, 1), src=[0], inc=[1 << 63], phi0=None, nsub=1, L=64, nbin=2)
    if name == "odd":                                    # 2: odd sizes, one unread tail sample, Ps = nbin, Ps > L
        x = int_data(3, 1000, 2)
        x[:, 999] = IN_GUARD
        inc = [ref.phase_step(p) for p in (7.0, 100.37, 33.3333, 999.5, 250.25)]
        assert inc[0] == ref.inc_limit(7)                # Ps = nbin: the largest step the kernel takes as given
        rng = np.random.default_rng(22)
        phi0 = [int(v) for v in rng.integers(0, 1 << 63, size=5)]
        phi0[1] = TWO64 - 3 * inc[1]
        phi0[2] = phi0[2] * 2 + 1
        return dict(x=x, src=[2, 0, 2, 1, 0], inc=inc, phi0=phi0, nsub=3, L=333, nbin=7)
    if name in ("chunks1024", "chunks256", "chunks64"):  # 3: three staging chunks, the last of one sample
        L = 2 * CH + 1
        x = int_data(2, 2 * L + 5, 3)
        x[:, 2 * L:] = IN_GUARD
        if name == "chunks64":
            # G = 4 threads a bin: they take turns up to a period of CH / G = 1024 samples and split
            # every run beyond (1024.0 and 1025.0: either side of the threshold); runs that span a
            # chunk boundary, a turn longer than a chunk and one longer than the sub-integration
            per = (1024.0, 1025.0, 1100.3, 3 * CH + 0.5, 40000.7, 64.0, 1023.99)
            rng = np.random.default_rng(33)
            return dict(x=x, src=[0, 1, 1, 0, 1, 0, 0], inc=[ref.phase_step(p) for p in per],
                        phi0=[int(v) * 2 + 1 for v in rng.integers(0, 1 << 63, size=7)], nsub=2, L=L, nbin=64)
        if name == "chunks1024":
            return dict(x=x, src=[0, 1, 1], inc=[ref.phase_step(1024.0), ref.phase_step(1500.7), 1 << 54],
                        phi0=[0, 12345678901234567, (1 << 64) - 1], nsub=2, L=L, nbin=1024)
        # a run of (3 CH + 0.5) / 256 = 48 samples per bin, a turn longer than a sub-integration
        return dict(x=x, src=[1, 0], inc=[ref.phase_step(3 * CH + 0.5)] * 2, phi0=[0, (1 << 63) + 99], nsub=2, L=L,
                    nbin=256)
    if name == "grid":                                   # 4: 333 workgroups
        rng = np.random.default_rng(4)
        per = np.exp(rng.uniform(np.log(64.0), np.log(3000.0), size=37))
        per[0], per[1] = 64.0, 700.0
        return dict(x=int_data(13, 9 * 700 + 3, 4), src=[int(v) for v in rng.integers(0, 13, size=37)],
                    inc=[ref.phase_step(p) for p in per], phi0=[int(v) * 2 + 1 for v in rng.integers(0, 1 << 63, 37)],
                    nsub=9, L=700, nbin=64)
    raise KeyError(name)


@kh.once
def reference(name):
    """A case and its float64 oracle (out, hits), computed once and shared (read-only)."""
    c = _case(name)
    return (c,) + ref.fold_series(c["x"], c["src"], c["inc"], c["phi0"], c["nsub"], c["L"], c["nbin"])[:2]


def _u64(vals):
    import torch
    return torch.from_numpy(np.array([v % TWO64 for v in vals], dtype=np.uint64).view(np.int64)).cuda()


def run_kernel(hip_lib, x, src, inc, phi0, nsub, L, nbin, ld=None, in_off=0, out_off=0, want_hits=True, nser=None):
    """pss_fold_series on views inside larger tensors (tests/kernel_harness.py):
    ``x`` with row stride ld behind a guard of at least five rows (+ in_off
    floats), ``out`` and ``hits`` flat.  Returns (out, hits)
    [nrows][nsub][nbin] after checking that nothing outside them was written."""
    import torch
    from psrsigsim_amd import _lib
    n, T = x.shape
    nser = n if nser is None else nser
    nrows = len(src)
    ld = T + 5 if ld is None else ld
    assert ld > T
    xin = kh.GuardedInput(x, ld, in_off, IN_GUARD, pad=max(kh.IN_PAD, 5 * ld))
    tot = nrows * nsub * nbin
    out = kh.GuardedOutput(1, tot, out_off=out_off, guard=OUT_GUARD)
    hits = kh.GuardedOutput(1, tot, out_off=out_off, guard=HIT_GUARD, dtype=np.int32)
    src_d = torch.from_numpy(np.array(src, dtype=np.int32)).cuda()
    inc_d = _u64(inc)
    phi_d = None if phi0 is None else _u64(phi0)
    rc = hip_lib.pss_fold_series(xin.ptr, nser, T, ld, src_d.data_ptr(), inc_d.data_ptr(),
                                 None if phi_d is None else phi_d.data_ptr(), nrows, nsub, L, nbin, out.ptr,
                                 hits.ptr if want_hits else None, None)
    _lib.check(rc, "fold_series")
    torch.cuda.synchronize()
    if not want_hits:
        hits.untouched()
    shape = (nrows, nsub, nbin)
    return out.read().reshape(shape), hits.read().reshape(shape)


def run_case(hip_lib, c, **kw):
    return run_kernel(hip_lib, c["x"], c["src"], c["inc"], c["phi0"], c["nsub"], c["L"], c["nbin"], **kw)


KERNEL_CASES = ["one", "odd", "chunks1024", "chunks256", "chunks64", "grid"]


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_index_cases_equal_the_oracle(name, hip_lib):
    c, out, hits = reference(name)
    T = c["x"].shape[1]
    assert c["nsub"] * c["L"] <= T
    if name == "one":
        assert np.array_equal(hits, [[[32, 32]]])
        assert np.array_equal(out[0, 0], [c["x"][0, 0::2].sum(), c["x"][0, 1::2].sum()])
    if name == "odd":
        assert (hits[0] > 0).all()                          # Ps = nbin: every bin of every turn
        assert (hits[3] == 0).sum() >= 3 * 3                # Ps = 999.5 > L: most of a sub-integration's bins are empty
        assert (out[3][hits[3] == 0] == 0).all()
    if name == "grid":
        assert len(c["src"]) * c["nsub"] == 333
    got, gh = run_case(hip_lib, c, ld=(T + 3) // 4 * 4 + 4)   # rows on the 16-B grid
    assert np.array_equal(gh, hits)
    assert (gh.sum(axis=2) == c["L"]).all()
    assert np.array_equal(got.astype(np.float64), out)


@pytest.mark.parametrize("name", ["odd", "chunks1024", "chunks256", "chunks64"])
def test_misaligned_views_give_the_same_bits(name, hip_lib):
    """The series view 1, 2 and 3 floats off the 16-B grid with an odd ld and
    out one float off: bitwise equal to the aligned run."""
    c, out, hits = reference(name)
    T = c["x"].shape[1]
    base, bh = run_case(hip_lib, c, ld=(T + 3) // 4 * 4 + 4)
    assert np.array_equal(base.astype(np.float64), out) and np.array_equal(bh, hits)
    odd = T + 1 + (T % 2)
    assert odd % 2 == 1 and odd > T
    for kw in (dict(ld=odd, in_off=1, out_off=1), dict(ld=odd, in_off=2, out_off=1),
               dict(ld=odd, in_off=3, out_off=1), dict(ld=(T + 3) // 4 * 4 + 4, in_off=1, out_off=0),
               dict(ld=odd, in_off=0, out_off=0)):
        got, gh = run_case(hip_lib, c, **kw)
        assert got.tobytes() == base.tobytes(), kw
        assert np.array_equal(gh, hits), kw


def test_clamps(hip_lib):
    """src below 0 and past the last series, and an inc above floor(2^64 /
    nbin), give the rows of the clamped values (and read nothing else)."""
    c, _, _ = reference("odd")
    x, nser = c["x"], 3
    lim = ref.inc_limit(7)
    src = [-1, nser + 3, -(1 << 31), (1 << 31) - 1, 1]
    inc = [c["inc"][1], c["inc"][2], lim + 12345, TWO64 - 1, lim + 1]
    want, wh, _ = ref.fold_series(x, [0, 2, 0, 2, 1], [inc[0], inc[1], lim, lim, lim], c["phi0"], 3, 333, 7)
    got, gh = run_kernel(hip_lib, x, src, inc, c["phi0"], 3, 333, 7)
    assert np.array_equal(gh, wh) and np.array_equal(got.astype(np.float64), want)
    assert (gh.sum(axis=2) == 333).all()
    # inc = 0 is valid: every sample in the bin of phi0
    got, gh = run_kernel(hip_lib, x, [1], [0], [11 * (TWO64 // 14)], 3, 333, 7)
    want, wh, _ = ref.fold_series(x, [1], [0], [11 * (TWO64 // 14)], 3, 333, 7)
    assert (wh[0, :, 5] == 333).all() and np.array_equal(gh, wh) and np.array_equal(got.astype(np.float64), want)


def _real(name):
    c, _, _ = reference(name)
    x = np.random.default_rng(7).standard_normal(c["x"].shape).astype(np.float32)
    return dict(c, x=x)


@pytest.mark.parametrize("name", ["odd", "grid", "chunks64"])
def test_real_data_within_the_derived_bound(name, hip_lib):
    """Standard-normal data against the float64 reference: |got - ref| <=
    2^-24 |ref| + n_b 2^-53 A_b, n_b the bin's hits and A_b its sum of |x| --
    the final rounding plus the worst case of a float64 accumulation in any
    order (derived, not measured).  No element is excluded."""
    c = _real(name)
    want, wh, mag = ref.fold_series(c["x"], c["src"], c["inc"], c["phi0"], c["nsub"], c["L"], c["nbin"])
    got, gh = run_case(hip_lib, c)
    assert np.array_equal(gh, wh)
    err = np.abs(got.astype(np.float64) - want)
    bound = 2.0 ** -24 * np.abs(want) + wh * 2.0 ** -53 * mag
    ok = bound > 0
    print("real data: max err / bound", float((err[ok] / bound[ok]).max()), "empty bins", int((~ok).sum()))
    assert (err <= bound).all()


def test_invariance(hip_lib):
    """Two runs give the same bits; a row alone gives the bits it has as row
    6 of a table of 9 other rows; hits = NULL leaves out unchanged."""
    for name in ("odd", "grid", "chunks64"):
        c = _real(name)
        a, ah = run_case(hip_lib, c)
        b, bh = run_case(hip_lib, c)
        assert a.tobytes() == b.tobytes() and ah.tobytes() == bh.tobytes()
        nohits, _ = run_case(hip_lib, c, want_hits=False)
        assert nohits.tobytes() == a.tobytes()
        r = 3
        one = dict(c, src=[c["src"][r]], inc=[c["inc"][r]], phi0=[c["phi0"][r]])
        alone, alh = run_case(hip_lib, one)
        assert alone[0].tobytes() == a[r].tobytes() and np.array_equal(alh[0], ah[r])
        n = len(c["src"])
        others = [(r + 1 + i) % n for i in range(9)]
        others = [o for o in others if o != r][:9]
        rows = others[:6] + [r] + others[6:9]
        many = dict(c, src=[c["src"][i] for i in rows], inc=[c["inc"][i] for i in rows],
                    phi0=[c["phi0"][i] for i in rows])
        if name == "grid":
            assert len(rows) == 10 and rows[6] == r
        among, amh = run_case(hip_lib, many)
        assert among[rows.index(r)].tobytes() == a[r].tobytes() and np.array_equal(amh[rows.index(r)], ah[r])


# ---------------------------------------------------------------------------
# API
# ---------------------------------------------------------------------------
def test_api_cube_equals_the_oracle_of_the_subband_sums(hip_lib):
    import torch
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.telescope import Backend, FoldedCandidates
    be = kh.backend()
    sig = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False)
    dms = [0.0, 10.0, 10.0, 5.0]
    ps_want = np.array([7.5, 100.37, 33.3333, 250.25])
    periods = ps_want / 1e4
    udms = np.array([0.0, 5.0, 10.0])
    ju = [0, 2, 2, 1]
    delays = Backend.dedisperse_delays(sig, udms)
    md = int(delays.max())
    assert 100 < md < 200
    T, nsub, L, nbin, nband, Cb = 1000, 3, 333, 7, 4, 16
    N = T + md
    data = int_data(64, N, 9)
    sig._buf = torch.from_numpy(data).cuda()
    sig._ncols = sig._nsamp = N
    fc = be.fold_candidates(sig, dms=dms, periods=periods, nbin=nbin, nsub=nsub, nband=nband, stat_block=128)
    assert isinstance(fc, FoldedCandidates) and len(fc) == 4
    assert tuple(fc.cube.shape) == (4, nband, nsub, nbin) and fc.cube.dtype == torch.float32 and fc.cube.is_cuda
    assert tuple(fc.hits.shape) == (4, nsub, nbin) and fc.hits.dtype == torch.int32
    assert tuple(fc.mean.shape) == tuple(fc.var.shape) == (4, nband) and fc.mean.dtype == torch.float64
    assert fc.T == T and fc.L == L and fc.max_delay == md and fc.ref_freq == 1593.75 and fc.samprate == 0.01
    ps = periods * (0.01 * 1e6)
    assert np.array_equal(fc.period_samples, ps) and np.allclose(ps, ps_want, rtol=1e-15)
    assert fc.inc == [ref.phase_step(v) for v in ps] and np.array_equal(fc.dms, dms)
    # the sub-band series in NumPy, from the table
    sub = np.zeros((nband, 3, T))
    for g in range(nband):
        for j in range(3):
            for c in range(g * Cb, (g + 1) * Cb):
                sub[g, j] += data[c, delays[j, c]:delays[j, c] + T]
    cube = fc.cube.cpu().numpy().astype(np.float64)
    hits = fc.hits.cpu().numpy()
    for g in range(nband):
        want, wh, _ = ref.fold_series(sub[g], ju, fc.inc, None, nsub, L, nbin)
        assert np.array_equal(cube[:, g], want), g
        assert np.array_equal(hits, wh)
    assert (hits.sum(axis=2) == L).all()
    assert np.array_equal(fc.profile().cpu().numpy().astype(np.float64), cube.sum(axis=(1, 2)))
    # duplicate DMs share a series: candidates 1 and 2 differ only in their period
    assert be._fold_plan(sig, dms=dms, periods=periods, nbin=nbin, nsub=nsub, nband=nband)["ju"].tolist() == ju
    same = be.fold_candidates(sig, dms=[10.0, 10.0], periods=[periods[2], periods[1]], nbin=nbin, nsub=nsub,
                              nband=nband, stat_block=128)
    assert torch.equal(same.cube[0], fc.cube[2]) and torch.equal(same.cube[1], fc.cube[1])
    # the statistics are _trial_stats of the sub-band series
    ld = (T + 3) // 4 * 4
    st = torch.zeros((nband * 3, ld), dtype=torch.float32, device="cuda")
    st[:, :T] = torch.from_numpy(sub.reshape(nband * 3, T).astype(np.float32)).cuda()
    m, v = Backend._trial_stats(st[:, :T], ld, 128)
    for k in range(4):
        for g in range(nband):
            assert fc.mean[k, g] == m[g * 3 + ju[k]] and fc.var[k, g] == v[g * 3 + ju[k]]
    # one DM per chunk: the same bits
    tiny = be.fold_candidates(sig, dms=dms, periods=periods, nbin=nbin, nsub=nsub, nband=nband, stat_block=128,
                              max_bytes=nband * ld * 4)
    assert len(be._fold_plan(sig, dms=dms, periods=periods, nbin=nbin, nsub=nsub, nband=nband,
                             max_bytes=nband * ld * 4)["chunks"]) == 3
    assert torch.equal(tiny.cube, fc.cube) and torch.equal(tiny.hits, fc.hits)
    assert torch.equal(tiny.mean, fc.mean) and torch.equal(tiny.var, fc.var)
    assert sig.data.cpu().numpy().tobytes() == data.tobytes()           # the signal is left as it was


def test_api_end_to_end_pulsar(hip_lib):
    """make_pulses -> ISM.disperse(30) -> fold_candidates at DM 0, 30, 60 and
    P = 50 ms -> refine: the set-up of
    tests/test_gpu_periodicity.py::test_api_end_to_end_pulsar (64 channels at
    1400 +- 200 MHz, 10 kHz, P = 500 samples, DM 30, 1.6384 s; T = 15 635, the
    largest delay 749; nbin 32, nsub 4, nband 4, stat_block 128).

    The NumPy restatement on the CPU oracle's signal (oracle/pss_cpu.py,
    LegacyDraws seeds 0 .. 5) gives: at DM 30 all 16 (band, sub-integration)
    profiles peak in the same bin, 15; chi2 is 1.45e6 - 1.82e6 at DM 30 and
    6.0e3 - 1.06e4 at DM 0 and DM 60, a ratio above 135.  The device draws from
    another generator, so asserted is only: at DM 30 every (band,
    sub-integration) profile peaks within +-1 bin of the summed profile's
    peak; chi2[DM 30] >= 10 x max(chi2[DM 0], chi2[DM 60]) (the reference
    alone clears this by more than 13 x); drift == 0 and dm_shift == 0 at DM
    30.  And the blind chain: the strongest candidate of periodicity_search
    folds at DM 30, at a period within one spectral bin of 50 ms, into a
    profile with a single peak (the maximum exceeds twice the median)."""
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar
    from psrsigsim_amd.ism import ISM
    pss.seed(20250101)
    sig = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False)
    Pulsar(0.05, 1.0).make_pulses(sig, tobs=1.6384)
    ISM().disperse(sig, 30)
    be = kh.backend()
    fc = be.fold_candidates(sig, dms=[0, 30, 60], periods=[0.05] * 3, nbin=32, nsub=4, nband=4, stat_block=128)
    assert fc.T == 15635 and fc.max_delay == 749 and fc.L == 15635 // 4
    assert fc.inc == [36893488147419103] * 3 and np.array_equal(fc.period_samples, [500.0] * 3)
    res = fc.refine()
    cube = fc.cube.cpu().numpy().astype(np.float64)
    peak = int(np.argmax(cube[1].sum(axis=(0, 1))))
    peaks = np.argmax(cube[1], axis=2)                                   # [band][sub-integration]
    dist = np.minimum((peaks - peak) % 32, (peak - peaks) % 32)
    print("chi2", res["chi2"], "chi2_opt", res["chi2_opt"], "drift", res["drift"], "dm_shift", res["dm_shift"],
          "peak", peak, "peaks", peaks.tolist())
    assert (dist <= 1).all()
    assert res["chi2"][1] >= 10.0 * max(res["chi2"][0], res["chi2"][2])
    assert res["drift"][1] == 0 and res["dm_shift"][1] == 0
    assert res["peak_bin"][1] == peak and res["period_opt"][1] == 0.05 and res["dm_opt"][1] == 30.0
    # blind: dedisperse, search, fold the strongest candidate
    plane = be.dedisperse(sig, np.arange(0, 65, 5))
    cands = be.periodicity_search(plane, stat_block=128)
    top = be.fold_candidates(sig, candidates=cands, max_candidates=1, nbin=32, nsub=4, nband=4, stat_block=128)
    assert len(top) == 1 and top.dms[0] == 30.0
    assert abs(1.0 / top.periods[0] - 20.0) <= cands.cells.df
    prof = top.profile()[0].cpu().numpy().astype(np.float64)
    print("blind: period", top.periods[0], "profile max", prof.max(), "median", np.median(prof))
    assert prof.max() > 2.0 * np.median(prof)
