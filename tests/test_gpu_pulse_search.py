"""Single-pulse search of the DM-time plane on the GPU (``pss_boxcar_search``,
``Backend.boxcar_snr``, ``Backend.single_pulse_search``).

The oracle is the float32 NumPy restatement of the kernel's definition in
tests/pulse_search_ref.py (``boxcar_ref``): the same rounded operations in the
same order, so every kernel-level comparison is ``array_equal`` on the bits of
``snr`` and on ``code`` -- no tolerance, no excluded cell.  Every kernel-level
case gives the kernel views inside larger tensors (row strides ld > T and
out_ld > nq) whose guard regions hold a sentinel: the input's is 2^20 (a read
outside a row's [0, T) then wins a cell), the outputs' are checked untouched
afterwards, the columns [nq, out_ld) of every row included.

The kernel's tile (pss_boxsearch.hip): a workgroup owns 2048 start times of one
trial; widths up to 256 samples (nw <= 9) share one kernel, nw = 10 .. 13 have
one each; steps of 256 samples and more are summed in registers.
"""
import numpy as np
import pytest

from tests import kernel_harness as kh
from tests import pulse_search_ref as ref
from tests.kernel_harness import engine_seed_restored, same_bits  # noqa: F401 (the fixture is autouse here)

pytestmark = pytest.mark.gpu

TILE = 2048
IN_GUARD = float(1 << 20)
SNR_GUARD = -7.0
CODE_GUARD = -77
DMS13 = np.arange(0, 65, 5)


def int_data(ndm, T, seed):
    """Integer-valued float32 in [-8, 7]: every box sum is exact, ties abound."""
    return np.random.default_rng(seed).integers(-8, 8, size=(ndm, T)).astype(np.float32)


def _case(name):
    """(plane [ndm][T] float32, mean, rstd, nw) of the exact cases."""
    if name == "one":                                    # (a) a single sample
        return int_data(1, 1, 1), 0.0, 1.0, 1
    if name == "ragged":                                 # (b) ragged last cell
        return int_data(3, 1000, 2), 0.0, 1.0, 6
    if name in ("t2049", "t2047"):                       # (c) the widest box fits at t = 0 and 1 only, or never
        x = int_data(2, TILE + 1 if name == "t2049" else TILE - 1, 3)
        x[1] = 7.0                                       # z grows with the width: the widest box that fits wins
        return x, 0.0, 1.0, 12
    if name == "plateau":                                # (d) 4096 samples of 7 across three tiles
        x = int_data(2, 3 * TILE + 77, 5)
        x[1, 1000:1000 + 4096] = 7.0
        x[1, 999] = x[1, 1000 + 4096] = -8.0
        return x, 0.0, 1.0, 13
    raise KeyError(name)


@kh.once
def reference(name, cell):
    """A case and its restatement, computed once and shared (read-only)."""
    x, mean, rstd, nw = _case(name)
    return (x, mean, rstd, nw) + ref.boxcar_ref(x, mean, rstd, nw, cell)


def run_kernel(hip_lib, x, mean, rstd, nw, cell, ld=None, out_ld=None, in_off=0, out_off=0):
    """pss_boxcar_search on views inside larger tensors (tests/kernel_harness.py):
    ``plane`` with row stride ld between guards, ``snr`` / ``code`` with row
    stride out_ld.  Returns (snr, code) [ndm][nq] after checking that nothing
    outside [j][0 .. nq) was written."""
    import torch
    from psrsigsim_amd import _lib
    ndm, T = x.shape
    nq = -(-T // cell)
    ld = T + 5 if ld is None else ld
    out_ld = nq + 3 if out_ld is None else out_ld
    assert ld > T and out_ld > nq
    plane = kh.GuardedInput(x, ld, in_off, IN_GUARD)
    m = torch.from_numpy(np.broadcast_to(np.asarray(mean, dtype=np.float32), (ndm,)).copy()).cuda()
    r = torch.from_numpy(np.broadcast_to(np.asarray(rstd, dtype=np.float32), (ndm,)).copy()).cuda()
    snr = kh.GuardedOutput(ndm, nq, out_ld, out_off, SNR_GUARD)
    code = kh.GuardedOutput(ndm, nq, out_ld, out_off, CODE_GUARD, np.int32)
    rc = hip_lib.pss_boxcar_search(plane.ptr, ndm, T, ld, m.data_ptr(), r.data_ptr(), nw, cell, snr.ptr, code.ptr,
                                   out_ld, None)
    _lib.check(rc, "boxcar_search")
    torch.cuda.synchronize()
    return snr.read(), code.read()


EXACT = [("one", 16), ("ragged", 32), ("t2049", 32), ("t2047", 32), ("plateau", 32)] + \
        [(n, c) for n in ("t2049", "t2047", "plateau") for c in (16, 256, 2048)] + \
        [("t2049", 512), ("t2049", 1024)]      # exactly one wave per cell, and two (the shared cell reduction)


@pytest.mark.parametrize("name,cell", EXACT)
def test_exact_cases_equal_the_restatement(name, cell, hip_lib):
    x, mean, rstd, nw, snr, code = reference(name, cell)
    T = x.shape[1]
    nq = -(-T // cell)
    # rows on the 16-B grid (16-B loads of the window) with an odd out_ld
    ld = (T + 3) // 4 * 4 + 4
    got_s, got_c = run_kernel(hip_lib, x, mean, rstd, nw, cell, ld=ld, out_ld=nq + 1 + (nq % 2))
    assert np.array_equal(got_c, code)
    assert same_bits(got_s, snr)
    time, wl = ref.decode(got_c, cell)
    assert (time + (1 << wl.astype(np.int64)) <= T).all()         # every winner lies inside the row
    if name == "one":
        assert got_s.shape == (1, 1) and got_s[0, 0] == x[0, 0] and got_c[0, 0] == 0
    if name == "t2049":
        assert set(time[wl == 11].tolist()) <= {0, 1} and wl[1, 0] == 11 and time[1, 0] == 0
    if name == "t2047":
        assert wl.max() == 10 and wl[1, 0] == 10 and time[1, 0] == 0
    if name == "plateau":
        # the width-4096 box at the plateau's start wins its cell: 7 * 4096 * 2^-6
        q = 1000 // cell
        assert got_s[1, q] == 448.0 and got_c[1, q] == (12 << 16) | (1000 - q * cell)


@kh.once
def _float_case():
    rng = np.random.default_rng(17)
    mean = rng.uniform(-50.0, 200.0, size=17).astype(np.float32)
    sigma = rng.uniform(0.3, 30.0, size=17)
    rstd = (1.0 / sigma).astype(np.float32)
    x = (rng.standard_normal((17, 5000)) * sigma[:, None] + mean[:, None].astype(np.float64)).astype(np.float32)
    return (x, mean, rstd) + ref.boxcar_ref(x, mean, rstd, 10, 32)


def test_float_data_bitwise(hip_lib):
    """17 trials of Gaussian data with their own mean / rstd, T = 5000, ten
    widths: bitwise the restatement; two launches give the same bits."""
    x, mean, rstd, snr, code = _float_case()
    got_s, got_c = run_kernel(hip_lib, x, mean, rstd, 10, 32, ld=5004, out_ld=160)
    assert np.array_equal(got_c, code)
    assert same_bits(got_s, snr)
    assert len(np.unique(got_c >> 16)) >= 8                       # most widths win somewhere
    again_s, again_c = run_kernel(hip_lib, x, mean, rstd, 10, 32, ld=5004, out_ld=160)
    assert again_s.tobytes() == got_s.tobytes() and again_c.tobytes() == got_c.tobytes()


@pytest.mark.parametrize("name", ["ragged", "plateau", "float"])
def test_misaligned_views_give_the_same_bits(name, hip_lib):
    """plane base off by one float and an odd ld (element loads), outputs off
    by one and an odd out_ld: bitwise equal to the aligned run."""
    if name == "float":
        x, mean, rstd, snr, code = _float_case()
        nw = 10
    else:
        x, mean, rstd, nw, snr, code = reference(name, 32)
    T = x.shape[1]
    nq = -(-T // 32)
    Ta, qa = (T + 3) // 4 * 4, (nq + 15) // 16 * 16
    base_s, base_c = run_kernel(hip_lib, x, mean, rstd, nw, 32, ld=Ta + 4, out_ld=qa + 16)
    assert same_bits(base_s, snr) and np.array_equal(base_c, code)
    for kw in kh.misaligned_layouts(Ta + 4, qa + 16, kh.odd(T + 2), kh.odd(nq + 2)):
        got_s, got_c = run_kernel(hip_lib, x, mean, rstd, nw, 32, **kw)
        assert got_s.tobytes() == base_s.tobytes() and got_c.tobytes() == base_c.tobytes(), kw


@pytest.mark.parametrize("cell", [16, 32])
def test_special_values(cell, hip_lib):
    """One NaN, one +inf and one -inf sample, and a run of NaN that fills
    whole cells: the restatement.  A NaN never wins; an all-NaN cell gives
    -inf and code 0."""
    x = np.array(_float_case()[0][:3, :3000])
    mean, rstd = _float_case()[1][:3], _float_case()[2][:3]
    x[0, 700] = np.nan
    x[0, 1500] = np.inf
    x[0, 2500] = -np.inf
    x[1, 64:128] = np.nan
    x[2, 2100] = np.inf                       # +inf and -inf in one box: NaN
    x[2, 2110] = -np.inf
    snr, code = ref.boxcar_ref(x, mean, rstd, 8, cell)
    got_s, got_c = run_kernel(hip_lib, x, mean, rstd, 8, cell)
    assert np.array_equal(got_c, code)
    assert same_bits(got_s, snr)
    assert not np.isnan(got_s).any()
    q = 64 // cell
    assert (got_s[1, q:128 // cell] == -np.inf).all() and (got_c[1, q:128 // cell] == 0).all()
    assert got_s[0, 1500 // cell] == np.inf and got_c[0, 1500 // cell] == 1500 % cell   # the narrowest box
    assert np.isfinite(got_s[0, 700 // cell]) and np.isfinite(got_s[0, 2500 // cell])


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


def test_api_with_user_statistics(hip_lib):
    import torch
    from psrsigsim_amd.telescope import BoxcarPlane
    be = kh.backend()
    data = np.random.default_rng(8).integers(0, 16, size=(64, 4096)).astype(np.float32)
    plane = be.dedisperse(_signal(data), DMS13)
    T = 4096 - 749
    x = plane.data.cpu().numpy()
    assert x.shape == (13, T)
    cells = be.boxcar_snr(plane, nwidths=9, cell=64, mean=0, std=8)
    assert isinstance(cells, BoxcarPlane) and cells.plane is plane and cells.cell == 64
    nq = -(-T // 64)
    for t, dt in ((cells.snr, torch.float32), (cells.time, torch.int64), (cells.width_log2, torch.int32),
                  (cells.code, torch.int32)):
        assert tuple(t.shape) == (13, nq) and t.dtype == dt and t.is_cuda
    assert cells.snr.stride(1) == 1 and cells.snr.stride(0) % 16 == 0 and cells.snr.data_ptr() % 64 == 0
    for t in (cells.mean, cells.std):
        assert tuple(t.shape) == (13,) and t.dtype == torch.float64 and t.is_cuda
    assert (cells.mean.cpu().numpy() == 0).all() and (cells.std.cpu().numpy() == 8).all()
    snr, code = ref.boxcar_ref(x, 0.0, np.float32(0.125), 9, 64)
    assert same_bits(cells.snr.cpu().numpy(), snr)
    assert np.array_equal(cells.code.cpu().numpy(), code)
    time, wl = ref.decode(code, 64)
    assert np.array_equal(cells.time.cpu().numpy(), time) and np.array_equal(cells.width_log2.cpu().numpy(), wl)
    # per-trial arrays give the same as the scalars they repeat
    again = be.boxcar_snr(plane, nwidths=9, cell=64, mean=np.zeros(13), std=np.full(13, 8.0))
    assert torch.equal(again.snr, cells.snr) and torch.equal(again.code, cells.code)
    assert plane.data.cpu().numpy().tobytes() == x.tobytes()                 # the plane is left as it was


def test_api_device_statistics(hip_lib):
    """The statistics boxcar_snr measures itself: the block medians of the
    restatement to float64 rounding -- the device sums a block of n = 400 in
    another order, and either sum is off by at most n u sum|x| (u = 2^-53,
    |x| < 400): 1.8e-11 on a block mean, 7.2e-9 on a block's mean of squares,
    so 7.2e-9 + 2 * 400 * 1.8e-11 = 2.2e-8 on a block variance, twice that
    between the two -- a constant trial gets S/N 0, trailing samples do not
    enter, and the map is bitwise the restatement's for the statistics the
    device reports."""
    import torch
    from psrsigsim_amd.telescope import DedispersedPlane
    x = np.array(_float_case()[0][:5, :4500])
    x[3] = 2.5                                                     # no variance: rstd 0
    x[:, 4400:] += 1000.0                                          # past the last whole block of 400
    plane = DedispersedPlane(torch.from_numpy(x).cuda(), np.arange(5.0), np.zeros((5, 1), dtype=np.int32), 0.01,
                             1500.0, 0)
    cells = kh.backend().boxcar_snr(plane, nwidths=4, cell=32, stat_block=400)
    mean, var = ref.block_median_stats(x, 400)
    got_m, got_s = cells.mean.cpu().numpy(), cells.std.cpu().numpy()
    print("mean diff", np.abs(got_m - mean).max(), "variance diff", np.abs(got_s ** 2 - var).max())
    assert np.allclose(got_m, mean, rtol=0, atol=2 * 1.8e-11) and got_m[3] == 2.5 and got_s[3] == 0.0
    good = np.arange(5) != 3
    assert np.allclose(got_s[good] ** 2, var[good], rtol=1e-15, atol=2 * 2.2e-8)
    s = cells.snr.cpu().numpy()
    assert (s[3] == 0).all()
    r32 = np.where(got_s > 0, 1.0 / np.where(got_s > 0, got_s, 1.0), 0.0).astype(np.float32)
    snr, code = ref.boxcar_ref(x, got_m.astype(np.float32), r32, 4, 32)
    assert same_bits(s, snr) and np.array_equal(cells.code.cpu().numpy(), code)
    # the step of 1000 (> 33 sigma per sample, sigma <= 30) never entered the statistics
    assert (s[good, 4400 // 32 + 1:] > 20).all()


def three_bursts():
    """The issue's input: 64 x 16384 unit normals plus three dispersed bursts
    at DM 30 (row 6 of DMS13's table)."""
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.telescope import Backend
    sig = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False)
    d = Backend.dedisperse_delays(sig, DMS13)
    x = np.random.default_rng(100).standard_normal((64, 16384)).astype(np.float32)
    for t, w, a in ((2000, 1, 3.0), (6000, 8, 1.0), (11000, 64, 0.4)):
        for c in range(64):
            x[c, t + d[6][c]:t + d[6][c] + w] += np.float32(a)
    return x


def test_api_three_bursts(hip_lib):
    """Three bursts of widths 1, 8 and 64 at DM 30 in white noise,
    threshold 9, the device's own statistics.  The restatement (run here on the
    plane the device dedispersed, with float64 block medians) gives 3
    candidates -- (6, 11000, 64, 25.14), (6, 2000, 1, 23.55), (6, 6000, 8,
    22.48) -- no cell within 0.5 % of the threshold (the nearest are 9.10 and
    8.80) and each peak > 1 % above the rest of its cluster: conditions checked
    below, so the summation order of the float64 statistics cannot flip a
    cell.  The device must then give the same 3 (dm_index, time, width) and
    S/N within 1e-5 relative: two float32 roundings (mean, rstd; 2^-24 each)
    propagated, not a measured number."""
    be = kh.backend()
    plane = be.dedisperse(_signal(three_bursts()), DMS13)
    x = plane.data.cpu().numpy()
    want, snr, code = ref.search_ref(x, 9.0, 8, 32)
    print("restatement:", want)
    assert [c[1:4] for c in want] == [(6, 11000, 64), (6, 2000, 1), (6, 6000, 8)]
    assert [round(c[0], 2) for c in want] == [25.14, 23.55, 22.48]
    fin = snr[np.isfinite(snr)]
    print("nearest to the threshold:", fin[fin < 9].max(), fin[fin >= 9].min())
    assert not ((fin > 9.0 * 0.995) & (fin < 9.0 * 1.005)).any()
    # each peak leads the cells of its own cluster by > 1 %
    jj, qq = np.nonzero(snr >= 9.0)
    time, wl = ref.decode(code, 32)
    t, w, s = time[jj, qq], 1 << wl[jj, qq].astype(np.int64), snr[jj, qq]
    labels = ref.cluster_all_pairs(jj, t, w, 1, 0)
    for lab in np.unique(labels):
        top = np.sort(s[labels == lab])[::-1]
        assert top.size == 1 or top[1] < top[0] * 0.99, top[:2]
    got = be.single_pulse_search(plane, threshold=9.0, nwidths=8, cell=32)
    print("device:", got.array)
    assert len(got) == 3
    for g, wnt in zip(got.array, want):
        assert (int(g["dm_index"]), int(g["time"]), int(g["width"])) == wnt[1:4]
        assert abs(float(g["snr"]) - wnt[0]) <= 1e-5 * wnt[0]
        assert int(g["ncells"]) == wnt[4]
        assert g["dm"] == 30.0 and g["t_sec"] == (wnt[2] + wnt[3] / 2.0) / 0.01e6
    assert got.cells.plane is plane and tuple(got.cells.snr.shape) == snr.shape
    print("whole map bitwise equal:", same_bits(got.cells.snr.cpu().numpy(), snr),
          np.array_equal(got.cells.code.cpu().numpy(), code))
    with pytest.raises(ValueError, match="threshold 1 exceed max_cells 10"):
        be.single_pulse_search(plane, threshold=1.0, max_cells=10)


def test_api_end_to_end_pulsar(hip_lib):
    """make_pulses -> ISM.disperse(30) -> dedisperse -> single_pulse_search(6):
    a 50 ms pulsar in 1.6384 s gives one candidate per period.  The CPU oracle
    over 12 seeds gives 32-33 candidates, 30-31 of them (>= 0.909) at DM index
    6, every width 64 or 128, the weakest S/N 6.1-8.0; the device draws from
    another generator, so: 28-36 candidates, >= 80 % at index 6, widths in
    {64, 128}."""
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar
    from psrsigsim_amd.ism import ISM
    pss.seed(20250101)
    sig = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False)
    Pulsar(0.05, 1.0).make_pulses(sig, tobs=1.6384)
    ISM().disperse(sig, 30)
    be = kh.backend()
    plane = be.dedisperse(sig, DMS13)
    got = be.single_pulse_search(plane, threshold=6.0)
    n = len(got)
    at6 = int((got.dm_index == 6).sum())
    print("candidates", n, "at DM index 6:", at6, "widths", sorted(set(got.width.tolist())),
          "weakest S/N", float(got.snr.min()) if n else None)
    print(got.array)
    assert 28 <= n <= 36
    assert at6 >= 0.8 * n
    assert set(got.width.tolist()) <= {64, 128}
