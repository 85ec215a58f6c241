"""The fast folding search on the GPU (``pss_ffa_scrunch``,
``pss_ffa_transform``, ``pss_ffa_profile_search``, ``Backend.ffa_snr``,
``Backend.ffa_search``).

The oracle is the float32 NumPy restatement of the kernels' definitions in
tests/ffa_ref.py: the same rounded operations in the same order, so every
kernel-level comparison is on the bits -- no tolerance, no excluded word.
Every kernel-level case gives the kernel views inside larger tensors whose
guard regions hold a sentinel (tests/kernel_harness.py): an input's is 2^20 (a
stray read lands in a sum, or wins a cell), an output's is checked untouched
afterwards, the words [m p, n) of a transform block included.

The transform's tile (pss_ffa.hip): the subtree below the first depth whose
nodes hold at most 8192 floats is computed by one workgroup in LDS; the levels
above it are one launch each.
"""
import numpy as np
import pytest

from tests import ffa_ref as ref
from tests import kernel_harness as kh
from tests import pulse_search_ref as psr
from tests.kernel_harness import engine_seed_restored, same_bits  # noqa: F401 (the fixture is autouse here)

pytestmark = pytest.mark.gpu

IN_GUARD = float(1 << 20)
OUT_GUARD = -7.0
INT_GUARD = -77
DMS13 = np.arange(0, 65, 5)


def series(kind, nser, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "int":
        return rng.integers(-8, 8, size=(nser, n)).astype(np.float32)
    return (rng.standard_normal((nser, n)) * 3.0 + 1.5).astype(np.float32)


# ---------------------------------------------------------------------------
# scrunch
# ---------------------------------------------------------------------------
def run_scrunch(hip_lib, x, lf, sub=None, ld=None, y_ld=None, in_off=0, out_off=0):
    import torch
    from psrsigsim_amd import _lib
    nser, T = x.shape
    n = T >> lf
    ld = T + 5 if ld is None else ld
    y_ld = n + 3 if y_ld is None else y_ld
    xin = kh.GuardedInput(x, ld, in_off, IN_GUARD)
    y = kh.GuardedOutput(nser, n, y_ld, out_off, OUT_GUARD)
    s = None if sub is None else torch.from_numpy(np.asarray(sub, dtype=np.float32)).cuda()
    rc = hip_lib.pss_ffa_scrunch(xin.ptr, nser, T, ld, None if s is None else s.data_ptr(), lf, y.ptr, y_ld, None)
    _lib.check(rc, "ffa_scrunch")
    torch.cuda.synchronize()
    return y.read()


@pytest.mark.parametrize("lf", [0, 1, 5])
def test_scrunch_equals_the_restatement(lf, hip_lib):
    """T = 1003 is no multiple of 2^lf: the tail [n << lf, T) holds the
    sentinel and is not read.  sub NULL copies the bits (lf = 0) or sums the
    raw samples; given, it is subtracted first."""
    x = series("float", 3, 1003, 40 + lf)
    n = 1003 >> lf
    x[:, n << lf:] = IN_GUARD
    x[1, 7] = -0.0
    sub = np.array([1.25, -3.0, 0.0], dtype=np.float32)
    assert same_bits(run_scrunch(hip_lib, x, lf), ref.scrunch_ref(x, lf))
    want = ref.scrunch_ref(x, lf, sub)
    got = run_scrunch(hip_lib, x, lf, sub)
    assert same_bits(got, want) and not same_bits(got, ref.scrunch_ref(x, lf))
    for kw in kh.misaligned_layouts(1004, (n + 3) // 4 * 4 + 4, 1007, kh.odd(n + 2)):
        assert same_bits(run_scrunch(hip_lib, x, lf, sub, ld=kw["ld"], y_ld=kw["out_ld"], in_off=kw["in_off"],
                                     out_off=kw["out_off"]), want), kw


def test_scrunch_octave_from_octave(hip_lib):
    """lf + 1 from the raw series equals lf = 1, sub NULL, of octave lf: the same tree."""
    x = series("float", 2, 5003, 44)
    sub = np.array([0.5, 2.0], dtype=np.float32)
    prev = run_scrunch(hip_lib, x, 0, sub)
    for lf in range(1, 5):
        scratch = run_scrunch(hip_lib, x, lf, sub)
        assert same_bits(scratch, ref.scrunch_ref(x, lf, sub))
        prev = run_scrunch(hip_lib, prev, 1)
        assert same_bits(prev, scratch), lf
    # the deepest tree
    x = series("float", 1, (1 << 16) * 3 + 11, 45)
    assert same_bits(run_scrunch(hip_lib, x, 16, sub[:1]), ref.scrunch_ref(x, 16, sub[:1]))


# ---------------------------------------------------------------------------
# transform
# ---------------------------------------------------------------------------
def run_transform(hip_lib, y, p0, np_, ld=None, in_off=0, out_off=0):
    """pss_ffa_transform on views inside larger tensors.  Returns out
    [nser][np][n]: the words the kernel must not write hold OUT_GUARD (the
    surroundings of out and of work are asserted untouched)."""
    import torch
    from psrsigsim_amd import _lib
    nser, n = y.shape
    ld = n + 5 if ld is None else ld
    yin = kh.GuardedInput(y, ld, in_off, IN_GUARD)
    out = kh.GuardedOutput(1, nser * np_ * n, None, out_off, OUT_GUARD)
    work = kh.GuardedOutput(1, nser * np_ * n, None, out_off, OUT_GUARD)
    rc = hip_lib.pss_ffa_transform(yin.ptr, nser, n, ld, p0, np_, out.ptr, work.ptr, None)
    _lib.check(rc, "ffa_transform")
    torch.cuda.synchronize()
    work.read()
    return out.read().reshape(nser, np_, n)


def transform_input(kind, nser, n, p0, np_, seed):
    """A series whose samples no period of the call reads hold the sentinel."""
    y = series(kind, nser, n, seed)
    y[:, max(n // p * p for p in range(p0, p0 + np_)):] = IN_GUARD
    return y


@kh.once
def transform_case(kind, nser, n, p0, np_):
    y = transform_input(kind, nser, n, p0, np_, n * 7 + p0)
    return y, ref.transform_ref(y, p0, np_, fill=OUT_GUARD)


# (nser, n, p0, np): n < 2 p; m = 2 .. 33 at p = 37; p = 2 .. 4096 at m = 2 and 3; m = 33 .. 25 in one call, 5 series
SHAPES = [(2, 100, 64, 1)] + [(2, m * 37 + 5, 37, 1) for m in (2, 3, 7, 8, 9, 31, 32, 33)] + \
         [(1, m * p + 1, p, 1) for p in (2, 3, 64, 4096) for m in (2, 3)] + [(5, 1000, 30, 11)]


@pytest.mark.parametrize("nser,n,p0,np_", SHAPES)
def test_transform_equals_the_restatement(nser, n, p0, np_, hip_lib):
    for kind in ("int", "float"):
        y, want = transform_case(kind, nser, n, p0, np_)
        got = run_transform(hip_lib, y, p0, np_)
        assert same_bits(got, want), kind
        for pi in range(np_):                              # words [m p, n) of every block: untouched
            m = n // (p0 + pi)
            assert (got[:, pi, m * (p0 + pi):] == OUT_GUARD).all()
        if kind == "int":                                  # exact sums: every profile holds the block's samples once
            for pi in range(np_):
                p = p0 + pi
                m = n // p
                assert (got[:, pi, :m * p].reshape(nser, m, p).sum(axis=2) == y[:, None, :m * p].sum(axis=2)).all()


def test_transform_many_subtrees_and_levels(hip_lib):
    """m = 600 at p = 64 (subtrees of 75 rows at depth 3: eight workgroups in
    LDS, three global levels) and m = 1000, 999 at p = 7, 8 (one workgroup, ten
    levels in LDS); two launches give the same bits."""
    assert ref.fuse_depth(600, 64) == 3 and ref.fuse_depth(1000, 7) == 0 and ref.depth(600) == 10
    for kind in ("int", "float"):
        y, want = transform_case(kind, 1, 64 * 600 + 13, 64, 1)
        got = run_transform(hip_lib, y, 64, 1)
        assert same_bits(got, want), kind
        again = run_transform(hip_lib, y, 64, 1)
        assert again.tobytes() == got.tobytes()
    y, want = transform_case("float", 2, 7003, 7, 2)
    assert same_bits(run_transform(hip_lib, y, 7, 2), want)


def test_transform_misaligned_views_give_the_same_bits(hip_lib):
    y, want = transform_case("float", 5, 1000, 30, 11)
    base = run_transform(hip_lib, y, 30, 11, ld=1004)
    assert same_bits(base, want)
    for kw in kh.misaligned_layouts(1004, 0, 1007, 0):
        got = run_transform(hip_lib, y, 30, 11, ld=kw["ld"], in_off=kw["in_off"], out_off=kw["out_off"])
        assert got.tobytes() == base.tobytes(), kw
    # a block does not depend on the other periods and series of the call
    alone = run_transform(hip_lib, y[3:4], 33, 1)
    assert alone[0, 0].tobytes() == base[3, 3].tobytes()


# ---------------------------------------------------------------------------
# profile search
# ---------------------------------------------------------------------------
def run_search(hip_lib, prof, n, p0, np_, rstd, rm, nw, cell, out_ld=None, in_off=0, out_off=0):
    """pss_ffa_profile_search on views inside larger tensors.  Returns (snr,
    code, phase) [nser][np][nq] after checking that nothing else was written."""
    import torch
    from psrsigsim_amd import _lib
    nser = prof.shape[0]
    nq = -(-(n // p0) // cell)
    out_ld = nq + 3 if out_ld is None else out_ld
    pin = kh.GuardedInput(prof.reshape(1, -1), prof.size + 4, in_off, IN_GUARD)
    r = torch.from_numpy(np.broadcast_to(np.asarray(rstd, dtype=np.float32), (nser,)).copy()).cuda()
    w = torch.from_numpy(np.broadcast_to(np.asarray(rm, dtype=np.float32), (np_,)).copy()).cuda()
    snr = kh.GuardedOutput(nser * np_, nq, out_ld, out_off, OUT_GUARD)
    code = kh.GuardedOutput(nser * np_, nq, out_ld, out_off, INT_GUARD, np.int32)
    phase = kh.GuardedOutput(nser * np_, nq, out_ld, out_off, INT_GUARD, np.int32)
    rc = hip_lib.pss_ffa_profile_search(pin.ptr, nser, n, p0, np_, r.data_ptr(), w.data_ptr(), nw, cell, snr.ptr,
                                        code.ptr, phase.ptr, out_ld, None)
    _lib.check(rc, "ffa_profile_search")
    torch.cuda.synchronize()
    return tuple(o.read().reshape(nser, np_, nq) for o in (snr, code, phase))


def profiles(kind, nser, n, p0, np_, seed):
    """Profiles in the transform's layout; the words [m p, n) of a block hold the sentinel."""
    prof = series(kind, nser * np_, n, seed).reshape(nser, np_, n)
    for pi in range(np_):
        prof[:, pi, n // (p0 + pi) * (p0 + pi):] = IN_GUARD
    return prof


def check_search(hip_lib, prof, n, p0, np_, rstd, rm, nw, cell, **kw):
    want = ref.profile_search_ref(prof, n, p0, np_, rstd, rm, nw, cell)
    got = run_search(hip_lib, prof, n, p0, np_, rstd, rm, nw, cell, **kw)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    assert same_bits(got[0], want[0])
    return got


# (n, p0, np, nw, cell): p = 2 and 3 (k = 0 only, nw larger than fits; m no multiple of the cell); p = 64; m < cell;
# m = 33 .. 25 in one call (cells the later periods do not have); a cell of 2048; profiles a workgroup searches
SEARCH_SHAPES = [(71, 2, 1, 6, 16), (100, 3, 1, 11, 16), (64 * 20 + 5, 64, 1, 11, 16), (64 * 5, 64, 1, 6, 16),
                 (1000, 30, 11, 6, 16), (2 * 3000 + 1, 2, 2, 3, 2048), (1500 * 20 + 3, 1500, 2, 11, 16),
                 (4096 * 2, 4096, 1, 11, 32), (1024 * 37, 1023, 2, 10, 32)]


@pytest.mark.parametrize("n,p0,np_,nw,cell", SEARCH_SHAPES)
def test_search_equals_the_restatement(n, p0, np_, nw, cell, hip_lib):
    """Integer data (ties abound: the order (z, -k, -s, -phase) decides) and
    Gaussian data with per-series rstd and per-period rm."""
    rng = np.random.default_rng(n)
    rstd = rng.uniform(0.1, 2.0, size=3).astype(np.float32)
    rm = rng.uniform(0.05, 1.0, size=np_).astype(np.float32)
    snr, code, phase = check_search(hip_lib, profiles("int", 3, n, p0, np_, n + 1), n, p0, np_, 1.0, 1.0, nw, cell)
    shift, wl = ref.decode(code, cell)
    for pi in range(np_):
        p, m = p0 + pi, n // (p0 + pi)
        nqp = -(-m // cell)
        assert (shift[:, pi, :nqp] < m).all() and (phase[:, pi, :nqp] < p).all()
        assert ((2 << wl[:, pi, :nqp]) <= p).all() and (wl < nw).all()
        # the cells this period does not have
        assert (snr[:, pi, nqp:] == -np.inf).all() and (code[:, pi, nqp:] == 0).all() and (phase[:, pi, nqp:] == 0).all()
    check_search(hip_lib, profiles("float", 3, n, p0, np_, n + 2), n, p0, np_, rstd, rm, nw, cell)
    if (n, p0) == (64 * 20 + 5, 64):
        # a box of 32 bins is the widest that is valid at p = 64: a plateau of 40 bins is found with it
        prof = np.zeros((1, 1, n), dtype=np.float32)
        prof[0, 0, 3 * 64 + 20:3 * 64 + 60] = 1.0
        snr, code, phase = check_search(hip_lib, prof, n, p0, 1, 1.0, 1.0, 11, cell)
        assert code[0, 0, 0] == (5 << 16) | 3 and phase[0, 0, 0] == 20 and snr[0, 0, 0] == 32 * ref.psr.coef(5)
    if (n, p0) == (1000, 30):
        assert -(-(n // 40) // cell) == 2 and snr.shape[2] == 3


def test_search_wrapping_pulse(hip_lib):
    """A two-bin pulse on bins p - 1 and 0 is found at phase p - 1 with k = 1."""
    n, p = 37 * 20, 37
    prof = series("float", 1, n, 3).reshape(1, 1, n) * np.float32(0.01)
    prof[0, 0, 5 * p + p - 1] = 10.0
    prof[0, 0, 5 * p] = 10.0
    snr, code, phase = check_search(hip_lib, prof, n, p, 1, 1.0, 1.0, 6, 16)
    assert code[0, 0, 0] == (1 << 16) | 5 and phase[0, 0, 0] == p - 1


def test_search_special_values(hip_lib):
    """NaN, +inf and -inf samples, +inf and -inf in one box, and a cell of NaN
    alone: a NaN never wins, an all-NaN cell gives -inf, 0, 0."""
    n, p, cell = 64 * 48, 64, 16
    prof = profiles("float", 2, n, p, 1, 9)
    prof[0, 0, 2 * p + 7] = np.nan
    prof[0, 0, 20 * p + 9] = np.inf
    prof[0, 0, 40 * p + 11] = -np.inf
    prof[1, 0, 16 * p:32 * p] = np.nan                      # the whole of cell 1
    prof[1, 0, 3 * p + 5] = np.inf
    prof[1, 0, 3 * p + 6] = -np.inf
    snr, code, phase = check_search(hip_lib, prof, n, p, 1, [0.5, 2.0], 0.25, 6, cell)
    assert not np.isnan(snr).any()
    assert snr[1, 0, 1] == -np.inf and code[1, 0, 1] == 0 and phase[1, 0, 1] == 0
    assert snr[0, 0, 1] == np.inf and code[0, 0, 1] == 4 and phase[0, 0, 1] == 9       # the narrowest box, shift 20
    assert np.isfinite(snr[0, 0, 0]) and np.isfinite(snr[0, 0, 2]) and snr[1, 0, 0] == np.inf


def test_search_misaligned_views_give_the_same_bits(hip_lib):
    n, p0, np_ = 1000, 30, 11
    prof = profiles("float", 3, n, p0, np_, 21)
    base = check_search(hip_lib, prof, n, p0, np_, 0.5, 0.2, 6, 16, out_ld=16)
    for kw in kh.misaligned_layouts(0, 16, 0, 5):
        got = run_search(hip_lib, prof, n, p0, np_, 0.5, 0.2, 6, 16, out_ld=kw["out_ld"], in_off=kw["in_off"],
                         out_off=kw["out_off"])
        assert all(g.tobytes() == b.tobytes() for g, b in zip(got, base)), kw


# ---------------------------------------------------------------------------
# API
# ---------------------------------------------------------------------------
def _signal(data):
    import torch
    from psrsigsim_amd.signal import FilterBankSignal
    sig = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False)
    sig._buf = torch.from_numpy(np.array(data)).cuda()
    sig._ncols = sig._nsamp = data.shape[1]
    return sig


def _plane(x):
    import torch
    from psrsigsim_amd.telescope import DedispersedPlane
    return DedispersedPlane(torch.from_numpy(x).cuda(), np.arange(float(x.shape[0])),
                            np.zeros((x.shape[0], 1), dtype=np.int32), 0.01, 1500.0, 0)


def _equal_maps(cells, maps):
    assert same_bits(cells.snr.cpu().numpy(), maps["snr"])
    for name in ("code", "phase", "shift", "width_log2", "period"):
        assert np.array_equal(getattr(cells, name).cpu().numpy(), maps[name]), name
    assert np.array_equal(cells.columns, maps["columns"])


def test_api_with_user_statistics(hip_lib):
    """Two octaves (lf 0: p 64 .. 127, lf 1: p 64 .. 100) of 5 trials of 4501
    samples: the maps are bitwise the restatement's, whole trials a chunk, two
    trials a chunk or runs of ten periods of one trial."""
    import torch
    from psrsigsim_amd.telescope import FFAPlane
    be = kh.backend()
    x = series("float", 5, 4501, 60)
    plane = _plane(x)
    cells = be.ffa_snr(plane, 0.0064, 0.02, bins=64, mean=1.5, std=3.0)
    assert isinstance(cells, FFAPlane) and cells.plane is plane and cells.cell == 16
    assert [(o["lf"], o["n"], o["p0"], o["np"]) for o in cells.plan] == [(0, 4501, 64, 64), (1, 2250, 64, 37)]
    ncols = cells.columns.shape[0]
    assert ncols == sum(-(-(4501 // p) // 16) for p in range(64, 128)) + sum(-(-(2250 // p) // 16)
                                                                              for p in range(64, 101))
    for t, dt in ((cells.snr, torch.float32), (cells.code, torch.int32), (cells.phase, torch.int32),
                  (cells.shift, torch.int64), (cells.width_log2, torch.int32), (cells.period, torch.float64)):
        assert tuple(t.shape) == (5, ncols) and t.dtype == dt and t.is_cuda
    assert (cells.mean.cpu().numpy() == 1.5).all() and (cells.std.cpu().numpy() == 3.0).all()
    maps = ref.snr_ref(x, 1e4, 0.0064, 0.02, np.float32(1.5), np.float32(1.0 / 3.0), bins=64)
    _equal_maps(cells, maps)
    assert np.isfinite(maps["snr"]).all() and len(np.unique(maps["width_log2"])) >= 4
    for mb in (8 * 4501 * 64 * 2, 8 * 4501 * 10):
        again = be.ffa_snr(plane, 0.0064, 0.02, bins=64, mean=np.full(5, 1.5), std=np.full(5, 3.0), max_bytes=mb)
        for name in ("snr", "code", "phase", "shift", "width_log2", "period"):
            assert torch.equal(getattr(again, name), getattr(cells, name)), (mb, name)
    assert plane.data.cpu().numpy().tobytes() == x.tobytes()                 # the plane is left as it was


def test_api_device_statistics(hip_lib):
    """The statistics ffa_snr measures itself are those of boxcar_snr (the
    bounds of tests/test_gpu_pulse_search.py::test_api_device_statistics: blocks
    of 400, |x| < 400); a constant trial gets S/N 0; and the maps are bitwise
    the restatement's for the statistics the device reports."""
    x = series("float", 4, 4500, 61) * np.float32(4.0)
    x[2] = 2.5                                                     # no variance: rstd 0
    x[:, 4400:] += 100.0                                           # past the last whole block of 400
    cells = kh.backend().ffa_snr(_plane(x), 0.0064, 0.0127, bins=64, stat_block=400)
    mean, var = psr.block_median_stats(x, 400)
    got_m, got_s = cells.mean.cpu().numpy(), cells.std.cpu().numpy()
    print("mean diff", np.abs(got_m - mean).max(), "variance diff", np.abs(got_s ** 2 - var).max())
    assert np.allclose(got_m, mean, rtol=0, atol=2 * 1.8e-11) and got_m[2] == 2.5 and got_s[2] == 0.0
    good = np.arange(4) != 2
    assert np.allclose(got_s[good] ** 2, var[good], rtol=1e-15, atol=2 * 2.2e-8)
    r32 = np.where(got_s > 0, 1.0 / np.where(got_s > 0, got_s, 1.0), 0.0).astype(np.float32)
    maps = ref.snr_ref(x, 1e4, 0.0064, 0.0127, got_m.astype(np.float32), r32, bins=64)
    _equal_maps(cells, maps)
    assert (cells.snr.cpu().numpy()[2] == 0).all()


TRAIN_AMP = 0.25


def pulse_train():
    """64 x 16384 unit normals (the recipe of test_gpu_pulse_search.three_bursts)
    plus a dispersed periodic pulse train at DM 30 (row 6 of DMS13's table):
    period 250.37 samples, pulse k on the three samples from floor(250.37 k + 0.5)."""
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.telescope import Backend
    sig = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False)
    d = Backend.dedisperse_delays(sig, DMS13)
    x = np.random.default_rng(100).standard_normal((64, 16384)).astype(np.float32)
    for k in range(int(16384 / 250.37) + 1):
        t = int(np.floor(k * 250.37 + 0.5))
        for c in range(64):
            x[c, t + d[6][c]:t + d[6][c] + 3] += np.float32(TRAIN_AMP)
    return x


def test_api_pulse_train(hip_lib):
    """A pulse train of period 250.37 samples and width 3 at DM 30 in white
    noise, searched from 200 to 300 samples with 128 bins (two octaves: p = 200
    .. 255 of the raw series, T = 15635, m = 78 .. 61, and p = 128 .. 150 of the
    series scrunched by two), threshold 8, the device's own statistics.
    The amplitude is chosen so that the restatement (run here on the plane the
    device dedispersed, with float64 block medians) puts its top candidate at
    trial 6 within one shift step of the truth, 250.37 = 250 + s / 61 at s =
    22.6, and has no cell within 0.5 % of the threshold: conditions checked
    below, so the summation order of the float64 statistics cannot flip a cell.
    The device must then give the same candidates with S/N within 1e-5
    relative: two float32 roundings (mean, rstd; 2^-24 each) propagated."""
    be = kh.backend()
    plane = be.dedisperse(_signal(pulse_train()), DMS13)
    x = plane.data.cpu().numpy()
    T = x.shape[1]
    assert T == 15635
    want, maps = ref.search_ref(x, 1e4, 0.02, 0.03, 8.0, bins=128)
    print("restatement:", want[:5], len(want))
    top = want[0]
    step = 1.0 / (T // 250 - 1) / 1e4                             # one shift at p = 250, in seconds
    assert top[1] == 6 and abs(top[2] - 250.37 / 1e4) <= step and top[5] == 250
    fin = maps["snr"][np.isfinite(maps["snr"])]
    print("nearest to the threshold:", fin[fin < 8].max(), fin[fin >= 8].min())
    assert not ((fin > 8.0 * 0.995) & (fin < 8.0 * 1.005)).any()
    got = be.ffa_search(plane, 0.02, 0.03, threshold=8.0, bins=128)
    print("device:", got.array[:5], len(got))
    assert len(got) == len(want)
    for g, w in zip(got.array, want):
        assert (int(g["dm_index"]), float(g["period"]), int(g["width"]), int(g["phase"]), int(g["bins"]),
                int(g["octave"]), int(g["shift"]), int(g["ncells"])) == w[1:]
        assert abs(float(g["snr"]) - w[0]) <= 1e-5 * w[0]
        assert g["dm"] == DMS13[w[1]] and g["freq"] == 1.0 / w[2] and g["width_sec"] == w[3] / 1e4
    assert got.cells.plane is plane and tuple(got.cells.snr.shape) == maps["snr"].shape
    print("whole map bitwise equal:", same_bits(got.cells.snr.cpu().numpy(), maps["snr"]))
    with pytest.raises(ValueError, match="threshold 1 exceed max_cells 10"):
        be.ffa_search(plane, 0.02, 0.03, threshold=1.0, bins=128, max_cells=10)


def test_api_end_to_end_pulsar(hip_lib):
    """make_pulses -> ISM.disperse(30) -> dedisperse -> ffa_search(40 .. 60 ms)
    -> fold_candidates: the set-up of
    tests/test_gpu_periodicity.py::test_api_end_to_end_pulsar (64 channels, 10
    kHz, P = 50 ms = 500 samples, DM 30, 1.6384 s, 13 trial DMs 0 .. 60, T =
    15635; no radiometer noise, hence stat_block = 128 as there).  Two octaves:
    p = 400 .. 511 of the raw series and p = 256 .. 300 of the series scrunched
    by two.  The restatement on the CPU oracle's signal (oracle/pss_cpu.py,
    LegacyDraws seeds 0 .. 11, dedispersed in NumPy) gives one candidate -- every
    cell above 8 joins one cluster of 3229 - 3503 cells, the pulsar has no noise
    -- at DM index 6, period 49.9967 - 50.0200 ms (p = 499 or 500), a box of 32
    bins, z = 3284 - 4239; the runner-up trial is 5 or 7 with a best z of 0.261
    - 0.358 of trial 6's.
    The device draws from another generator, so asserted is only: the top
    candidate is at DM index 6 with a period within 1 % of 50 ms, and folding it
    (fold_candidates takes the FFACandidates as they stand) gives a profile
    with a single peak (the maximum exceeds twice the median)."""
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar
    from psrsigsim_amd.ism import ISM
    from psrsigsim_amd.telescope import FFACandidates, PeriodCandidates
    pss.seed(20250101)
    sig = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False)
    Pulsar(0.05, 1.0).make_pulses(sig, tobs=1.6384)
    ISM().disperse(sig, 30)
    be = kh.backend()
    plane = be.dedisperse(sig, DMS13)
    got = be.ffa_search(plane, 0.04, 0.06, stat_block=128)
    assert isinstance(got, FFACandidates) and isinstance(got, PeriodCandidates) and len(got) >= 1
    assert [(o["lf"], o["p0"], o["np"]) for o in got.cells.plan] == [(0, 400, 112), (1, 256, 45)]
    per_trial = got.cells.snr.max(dim=1).values.cpu().numpy()
    print("candidates", len(got), "best", got[0], "best z per trial", per_trial)
    assert int(got[0]["dm_index"]) == 6 and abs(float(got[0]["period"]) - 0.05) <= 0.01 * 0.05
    top = be.fold_candidates(sig, candidates=got, max_candidates=1, nbin=32, nsub=4, nband=4, stat_block=128)
    assert len(top) == 1 and top.dms[0] == 30.0 and top.periods[0] == float(got[0]["period"])
    prof = top.profile()[0].cpu().numpy().astype(np.float64)
    print("folded: period", top.periods[0], "profile max", prof.max(), "median", np.median(prof), "bin", prof.argmax())
    assert prof.max() > 2.0 * np.median(prof)
