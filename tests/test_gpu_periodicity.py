"""Periodicity search of the DM-time plane on the GPU (``pss_harmonic_search``,
``Backend.dm_spectrum``, ``Backend.harmonic_snr``, ``Backend.periodicity_search``).

The oracle is the float32 NumPy restatement of the kernel's definition in
tests/periodicity_ref.py (``harmonic_ref``): the same rounded operations in the
same order, so every kernel-level comparison is ``array_equal`` on the bits of
``snr`` and on ``code`` -- no tolerance, no excluded cell.  Every kernel-level
case gives the kernel views inside larger tensors (row strides ld > nbin and
out_ld > nq) whose guard regions hold a sentinel: the input's is 1e30, around
every row and in its bins below kmin (a read outside [kmin, nbin) then wins a
cell with an infinite power; the restatement is given the clean spectrum), the
outputs' are checked untouched afterwards, the columns [nq, out_ld) of every
row included.

The kernel's tile (pss_harmsum.hip): a workgroup owns 2048 bins of one trial.
"""
import functools

import numpy as np
import pytest

from tests import kernel_harness as kh
from tests import periodicity_ref as ref
from tests import pulse_search_ref as psref
from tests.kernel_harness import engine_seed_restored, same_bits  # noqa: F401 (the fixture is autouse here)

pytestmark = pytest.mark.gpu

TILE = 2048
IN_GUARD = 1e30
SNR_GUARD = -7.0
CODE_GUARD = -77
WORK_GUARD = -3.0


def tri_data(ndm, nbin, seed):
    """re, im in {-1, 0, 1}: P in {0, 1, 2}, every sum exact, ties everywhere."""
    r = np.random.default_rng(seed).integers(-1, 2, size=(2, ndm, nbin)).astype(np.float32)
    return (r[0] + 1j * r[1]).astype(np.complex64)


def _case(name):
    """(spec [ndm][nbin] complex64, scale, nl, kmin) of the exact cases."""
    if name == "r2500":
        return tri_data(3, 2500, 1), 1.0, 5, 1
    if name.startswith("r2500_nl"):                      # fewer levels
        return tri_data(3, 2500, 1), 1.0, int(name[-1]), 1
    if name == "edges":                                  # tile edges at 2048 and 4096
        return tri_data(2, 2 * TILE + 1, 2), 1.0, 5, 1
    if name in ("edge-1", "edge+1"):
        return tri_data(2, TILE + (1 if name == "edge+1" else -1), 3), 1.0, 5, 1
    if name[0] == "s":                                   # s<nbin>_<kmin>: levels and cells with no valid bin
        nbin, kmin = (int(v) for v in name[1:].split("_"))
        return tri_data(1 if nbin == 17 else 2, nbin, 4 + nbin), 1.0, 5, kmin
    if name == "kmin700":                                # level l starts at k = 700 2^l - 2^(l-1); none at l = 4
        return tri_data(2, 3000, 5), 1.0, 5, 700
    if name == "trials":                                 # many trials, short rows
        return tri_data(70, 300, 6), 1.0, 5, 1
    if name in ("plateau", "plateau_k5"):                # all P = 1: every z is 0
        return np.ones((2, 2500), dtype=np.complex64), 1.0, 5, 5 if name == "plateau_k5" else 1
    raise KeyError(name)


@kh.once
def reference(name, cell):
    """A case and its restatement, computed once and shared (read-only)."""
    x, scale, nl, kmin = _case(name)
    return (x, scale, nl, kmin) + ref.harmonic_ref(x, scale, nl, kmin, cell)


def run_kernel(hip_lib, x, scale, nl, kmin, cell, ld=None, out_ld=None, in_off=0, out_off=0):
    """pss_harmonic_search on views inside larger tensors (tests/kernel_harness.py):
    ``spec`` with row stride ld complex elements between guards (in_off = 2 is
    one complex element, in_off = 1 half of one), ``snr`` / ``code`` with row
    stride out_ld; the bins below kmin hold the input guard too.  The kernel
    runs twice, without and with the workspace of its power pass, and must
    give the same bits.  Returns (snr, code) [ndm][nq] after checking that
    nothing outside [j][0 .. nq) was written."""
    import torch
    from psrsigsim_amd import _lib
    ndm, nbin = x.shape
    nq = -(-nbin // cell)
    ld = nbin + 5 if ld is None else ld
    out_ld = nq + 3 if out_ld is None else out_ld
    assert ld > nbin and out_ld > nq
    xs = np.array(x, dtype=np.complex64)
    xs[:, :min(kmin, nbin)] = IN_GUARD * (1 + 1j)
    spec = kh.GuardedInput(xs.view(np.float32).reshape(ndm, nbin, 2), ld, in_off, IN_GUARD)
    s = torch.from_numpy(np.broadcast_to(np.asarray(scale, dtype=np.float32), (ndm,)).copy()).cuda()
    res = []
    for with_work in (False, True):
        # the workspace of the power pass: ndm * nbin floats between guards of their own
        work = kh.GuardedOutput(ndm, nbin, guard=WORK_GUARD)
        snr = kh.GuardedOutput(ndm, nq, out_ld, out_off, SNR_GUARD)
        code = kh.GuardedOutput(ndm, nq, out_ld, out_off, CODE_GUARD, np.int32)
        rc = hip_lib.pss_harmonic_search(spec.ptr, ndm, nbin, ld, s.data_ptr(), nl, kmin, cell, snr.ptr, code.ptr,
                                         out_ld, work.ptr if with_work else None, None)
        _lib.check(rc, "harmonic_search")
        torch.cuda.synchronize()
        if not with_work:
            work.untouched()
        else:
            # the powers of the bins a sum may read, and nothing below kmin
            assert (work.read()[:, :min(kmin, nbin)] == WORK_GUARD).all()
        res.append((snr.read(), code.read()))
    # with and without the workspace: the same bits
    assert res[0][0].tobytes() == res[1][0].tobytes() and res[0][1].tobytes() == res[1][1].tobytes()
    return res[0]


EXACT = [("r2500", 16), ("r2500", 2048), ("edges", 32), ("edge-1", 32), ("edge+1", 32), ("edge+1", 512),
         ("edge+1", 2048), ("s1_1", 16), ("s1_3", 16), ("s7_1", 16), ("s7_3", 16), ("s17_1", 16), ("s17_3", 16),
         ("kmin700", 32), ("kmin700", 1024), ("trials", 32), ("plateau", 32), ("plateau_k5", 256),
         ("r2500_nl1", 32), ("r2500_nl2", 32), ("r2500_nl3", 32), ("r2500_nl4", 32)]


@pytest.mark.parametrize("name,cell", EXACT)
def test_exact_cases_equal_the_restatement(name, cell, hip_lib):
    x, scale, nl, kmin, snr, code = reference(name, cell)
    nbin = x.shape[1]
    nq = -(-nbin // cell)
    # rows on the 16-B grid with an odd out_ld
    got_s, got_c = run_kernel(hip_lib, x, scale, nl, kmin, cell, ld=(nbin + 1) // 2 * 2 + 2,
                              out_ld=nq + 1 + (nq % 2))
    assert np.array_equal(got_c, code)
    assert same_bits(got_s, snr)
    k, lev = ref.decode(got_c, cell)
    won = got_s > -np.inf
    assert (k[won] < nbin).all() and (lev[won] < nl).all()
    assert (((k + (1 << lev >> 1)) >> lev)[won] >= kmin).all()       # every winner's fundamental is at or above kmin
    assert (got_c[~won] == 0).all()
    if name == "s1_1":
        # bin 0 is never a fundamental
        assert got_s.shape == (2, 1) and (got_s == -np.inf).all()
    if name == "s7_3":
        # level 0 from k = 3, level 1 from k = 5, level 2 never ((k + 2) / 4 < 3 for k < 10)
        assert won.all() and lev.max() <= 1
    if name == "s17_3":
        # the second cell holds k = 16 alone: levels 0 .. 2 ((16 + 4) / 8 = 2 < 3)
        assert got_s.shape == (1, 2) and k[0, 1] == 16 and lev[0, 1] <= 2
    if name == "kmin700":
        # level l is valid from k = 700 2^l - 2^(l-1): 700, 1399, 2798 (inside a tile), then 5596 > nbin
        assert (got_s[:, :700 // cell] == -np.inf).all() and won[:, 700 // cell:].all()
        first = [700 * (1 << l) - (1 << l >> 1) for l in range(4)]
        assert first == [700, 1399, 2798, 5596] and lev.max() == 2
        assert all(k[won & (lev == l)].min() >= first[l] for l in range(3))
        assert (lev == 1).any() and (lev == 2).any()
    if name.startswith("r2500_nl"):
        assert lev.max() == nl - 1
    if name.startswith("plateau"):
        # every z is 0: level 0 and the first valid bin of every cell
        assert (got_s[won] == 0).all() and (lev == 0).all()
        q = np.arange(nq) * cell
        assert won.all() and np.array_equal(k[0], np.maximum(q, kmin)) and np.array_equal(k[1], k[0])


@kh.once
def _float_case():
    rng = np.random.default_rng(23)
    x = (rng.standard_normal((4, 6000)) + 1j * rng.standard_normal((4, 6000))).astype(np.complex64)
    scale = rng.uniform(0.5, 2.0, size=4).astype(np.float32)
    return x, scale, {nl: ref.harmonic_ref(x, scale, nl, 1, 32) for nl in range(1, 6)}


@pytest.mark.parametrize("nl", [1, 2, 3, 4, 5])
def test_float_data_bitwise(nl, hip_lib):
    """4 trials of 6000 complex normal values with their own scale: bitwise the
    restatement at every number of levels; two launches give the same bits."""
    x, scale, maps = _float_case()
    snr, code = maps[nl]
    got_s, got_c = run_kernel(hip_lib, x, scale, nl, 1, 32, ld=6004, out_ld=192)
    assert np.array_equal(got_c, code)
    assert same_bits(got_s, snr)
    assert len(np.unique(got_c >> 16)) == nl                      # every level wins somewhere
    if nl == 5:
        again_s, again_c = run_kernel(hip_lib, x, scale, nl, 1, 32, ld=6004, out_ld=192)
        assert again_s.tobytes() == got_s.tobytes() and again_c.tobytes() == got_c.tobytes()


@pytest.mark.parametrize("name", ["r2500", "kmin700", "float"])
def test_misaligned_views_give_the_same_bits(name, hip_lib):
    """The spectrum off by one complex element (8 B: off the 16-B grid) or by
    one float (4 B: dword loads), an odd ld, the maps off by one with an odd
    out_ld: bitwise equal to the aligned run."""
    if name == "float":
        x, scale, maps = _float_case()
        nl, kmin = 5, 1
        snr, code = maps[5]
    else:
        x, scale, nl, kmin, snr, code = reference(name, 32)
    nbin = x.shape[1]
    nq = -(-nbin // 32)
    na, qa = (nbin + 1) // 2 * 2, (nq + 15) // 16 * 16
    base_s, base_c = run_kernel(hip_lib, x, scale, nl, kmin, 32, ld=na + 2, out_ld=qa + 16)
    assert same_bits(base_s, snr) and np.array_equal(base_c, code)
    odd = kh.odd
    for kw in list(kh.misaligned_layouts(na + 2, qa + 16, odd(nbin + 2), odd(nq + 2), in_off=2)) + [
            dict(ld=odd(nbin + 2), out_ld=qa + 16, in_off=1, out_off=0),          # 4 B: off the 8-B grid
            dict(ld=na + 2, out_ld=odd(nq + 2), in_off=3, out_off=1)]:
        got_s, got_c = run_kernel(hip_lib, x, scale, nl, kmin, 32, **kw)
        assert got_s.tobytes() == base_s.tobytes() and got_c.tobytes() == base_c.tobytes(), kw


@pytest.mark.parametrize("cell", [16, 32])
def test_special_values(cell, hip_lib):
    """NaN, +-inf and 0 in the spectrum, a run of NaN over whole cells, and a
    trial with scale 0: the restatement.  A NaN never wins; a cell whose every
    sum holds a NaN gives -inf and code 0; the trial with scale 0 has P = 0
    (or NaN at an infinite bin) and z = -h a_l, largest at level 0."""
    x = np.array(_float_case()[0][:3, :3000])
    scale = np.array(_float_case()[1][:3])
    scale[2] = 0.0
    x[0, 700] = np.nan
    x[0, 1500] = np.inf
    x[0, 2500] = complex(0.0, -np.inf)
    x[0, 2900:2910] = 0.0
    x[1, 2048:2112] = complex(np.nan, 1.0)
    x[2, 100] = np.inf                          # inf * 0 = NaN in the trial with scale 0
    snr, code = ref.harmonic_ref(x, scale, 5, 1, cell)
    got_s, got_c = run_kernel(hip_lib, x, scale, 5, 1, cell)
    assert np.array_equal(got_c, code)
    assert same_bits(got_s, snr)
    assert not np.isnan(got_s).any()
    a, b = 2048 // cell, 2112 // cell
    assert (got_s[1, a:b] == -np.inf).all() and (got_c[1, a:b] == 0).all()
    assert got_s[0, 1500 // cell] == np.inf and got_c[0, 1500 // cell] == 1500 % cell     # the fewest harmonics
    assert got_s[0, 2500 // cell] == np.inf and np.isfinite(got_s[0, 700 // cell])
    fin = np.ones(got_s.shape[1], dtype=bool)
    fin[100 // cell] = False
    assert (got_s[2, fin] == -1.0).all() and (got_c[2, 1:][fin[1:]] == 0).all() and got_c[2, 0] == 1


# ---------------------------------------------------------------------------
# API
# ---------------------------------------------------------------------------
def _plane(x, dms=None):
    import torch
    from psrsigsim_amd.telescope import DedispersedPlane
    x = np.asarray(x, dtype=np.float32)
    dms = np.arange(float(x.shape[0])) if dms is None else dms
    return DedispersedPlane(torch.from_numpy(np.array(x)).cuda(), dms, np.zeros((x.shape[0], 1), dtype=np.int32),
                            0.01, 1500.0, 0)


@functools.lru_cache(maxsize=None)
def _series():
    """5 trials x 4500 samples of Gaussian data with their own mean and sigma."""
    rng = np.random.default_rng(31)
    mean = rng.uniform(-50.0, 200.0, size=5)
    sigma = rng.uniform(0.3, 30.0, size=5)
    x = (rng.standard_normal((5, 4500)) * sigma[:, None] + mean[:, None]).astype(np.float32)
    x.setflags(write=False)
    return x, mean, sigma


@pytest.mark.parametrize("nfft", [None, 4096, 9000, 3750])
def test_dm_spectrum_against_float64(nfft, hip_lib):
    """dm_spectrum against np.fft.rfft in float64 of the same float32 input
    (x - mean32, cut to min(T, nfft) samples, zero-padded to nfft): every bin
    of every row within 4 eps32 log2(nfft) ||x||_2, the standard bound of a
    float32 FFT (eps32 = 2^-23)."""
    import torch
    x, mean, _ = _series()
    be = kh.backend()
    plane = _plane(x)
    n = 4500 if nfft is None else nfft                                # fft_length(4500) = 4500 = 2^2 3^2 5^3
    spec = be.dm_spectrum(plane, nfft=nfft, mean=mean)
    assert spec.dtype == torch.complex64 and tuple(spec.shape) == (5, n // 2 + 1) and spec.is_cuda
    m32 = mean.astype(np.float32)
    y = x[:, :min(4500, n)] - m32[:, None]
    assert y.dtype == np.float32
    want = np.fft.rfft(y.astype(np.float64), n=n, axis=1)
    err = np.abs(spec.cpu().numpy().astype(np.complex128) - want).max(axis=1)
    bound = 4 * 2.0 ** -23 * np.log2(n) * np.sqrt((y.astype(np.float64) ** 2).sum(axis=1))
    print("nfft", n, "error / bound per row", err / bound)
    assert (err <= bound).all()
    # a subset of the trials is the same rows
    part = be.dm_spectrum(plane, nfft=nfft, mean=mean, trials=(1, 3))
    assert tuple(part.shape) == (2, n // 2 + 1)
    assert np.abs(part.cpu().numpy().astype(np.complex128) - want[1:3]).max(axis=1).max() <= bound[1:3].min()
    if nfft is None:
        # the default mean is the block median of the single-pulse search
        auto = be.dm_spectrum(plane)
        bm, _ = psref.block_median_stats(x, 1024)
        y2 = x - bm.astype(np.float32)[:, None]
        want2 = np.fft.rfft(y2.astype(np.float64), axis=1)
        b2 = 4 * 2.0 ** -23 * np.log2(n) * np.sqrt((y2.astype(np.float64) ** 2).sum(axis=1))
        # (the device's float64 block means differ from the host's by rounding: one float32 ulp of the mean,
        # 200 * 2^-24 * 4500 on bin 0, may come on top)
        assert (np.abs(auto.cpu().numpy().astype(np.complex128) - want2)[:, 1:].max(axis=1) <= b2).all()


def test_harmonic_snr_user_statistics(hip_lib):
    import torch
    from psrsigsim_amd.telescope import HarmonicPlane
    x, mean, sigma = _series()
    be = kh.backend()
    plane = _plane(x)
    spec = be.dm_spectrum(plane, mean=mean)
    cells = be.harmonic_snr(plane, nharm=8, cell=64, fmin=3.0, mean=mean, std=sigma, spectrum=spec)
    nbin, df = 2250, 1e4 / 4500
    nq = -(-nbin // 64)
    assert isinstance(cells, HarmonicPlane) and cells.plane is plane and cells.cell == 64
    assert (cells.nfft, cells.nbin, cells.kmin, cells.df) == (4500, nbin, 2, df)             # ceil(3 / 2.22) = 2
    for t, dt in ((cells.snr, torch.float32), (cells.bin, torch.int64), (cells.nharm_log2, torch.int32),
                  (cells.code, torch.int32), (cells.freq, torch.float64)):
        assert tuple(t.shape) == (5, nq) and t.dtype == dt and t.is_cuda
    assert cells.snr.stride(1) == 1 and cells.snr.stride(0) % 16 == 0 and cells.snr.data_ptr() % 64 == 0
    assert np.array_equal(cells.mean.cpu().numpy(), mean) and np.array_equal(cells.std.cpu().numpy(), sigma)
    scale = ref.scale_f32(sigma * sigma, 4500)
    snr, code = ref.harmonic_ref(spec.cpu().numpy()[:, :nbin], scale, 4, 2, 64)
    assert same_bits(cells.snr.cpu().numpy(), snr)
    assert np.array_equal(cells.code.cpu().numpy(), code)
    k, lev = ref.decode(code, 64)
    assert np.array_equal(cells.bin.cpu().numpy(), k) and np.array_equal(cells.nharm_log2.cpu().numpy(), lev)
    assert np.array_equal(cells.freq.cpu().numpy(), k / (1 << lev.astype(np.int64)).astype(np.float64) * df)
    # four harmonics and fewer take the kernel's other path (no workspace)
    four = be.harmonic_snr(plane, nharm=4, cell=64, fmin=3.0, mean=mean, std=sigma, spectrum=spec)
    snr4, code4 = ref.harmonic_ref(spec.cpu().numpy()[:, :nbin], scale, 3, 2, 64)
    assert same_bits(four.snr.cpu().numpy(), snr4) and np.array_equal(four.code.cpu().numpy(), code4)
    # the transform inside gives the same map, and so does one trial per chunk
    own = be.harmonic_snr(plane, nharm=8, cell=64, fmin=3.0, mean=mean, std=sigma)
    assert torch.equal(own.snr.view(torch.int32), cells.snr.view(torch.int32)) and torch.equal(own.code, cells.code)
    one = be.harmonic_snr(plane, nharm=8, cell=64, fmin=3.0, mean=mean, std=sigma, max_bytes=2251 * 8)
    assert be._harmonic_plan(plane, max_bytes=2251 * 8)["chunk"] == 1
    assert torch.equal(one.snr.view(torch.int32), cells.snr.view(torch.int32)) and torch.equal(one.code, cells.code)
    two = be.harmonic_snr(plane, nharm=8, cell=64, fmin=3.0, mean=mean, std=sigma, max_bytes=2 * 2251 * 8 + 100)
    assert torch.equal(two.snr.view(torch.int32), cells.snr.view(torch.int32)) and torch.equal(two.code, cells.code)
    assert plane.data.cpu().numpy().tobytes() == x.tobytes()                 # the plane is left as it was


def test_harmonic_snr_device_statistics_and_zero_padding(hip_lib):
    """The statistics harmonic_snr measures itself are those of boxcar_snr (the
    block medians of the restatement to float64 rounding; the bounds are
    derived in tests/test_gpu_pulse_search.py::test_api_device_statistics, here
    for blocks of n = 500 and |x| < 400: 2.3e-11 on a mean, 2 * (9e-9 + 2 * 400 *
    2.3e-11) = 5.4e-8 on a variance), a constant trial gets scale 0 -- every
    z = -1 at level 0 -- and the map is bitwise the restatement's for the
    statistics the device reports, at nfft = 2 T too."""
    x = np.array(_series()[0])
    x[3] = 2.5
    plane = _plane(x)
    be = kh.backend()
    for nfft, n in ((None, 4500), (9000, 9000)):
        cells = be.harmonic_snr(plane, nharm=16, cell=32, nfft=nfft, stat_block=500)
        mean, var = psref.block_median_stats(x, 500)
        got_m, got_s = cells.mean.cpu().numpy(), cells.std.cpu().numpy()
        print("mean diff", np.abs(got_m - mean).max(), "variance diff", np.abs(got_s ** 2 - var).max())
        assert np.allclose(got_m, mean, rtol=0, atol=2 * 2.3e-11) and got_m[3] == 2.5 and got_s[3] == 0.0
        good = np.arange(5) != 3
        assert np.allclose(got_s[good] ** 2, var[good], rtol=1e-15, atol=5.4e-8)
        assert cells.nfft == n and cells.nbin == n // 2 and cells.df == 1e4 / n
        spec = be.dm_spectrum(plane, nfft=nfft, mean=cells.mean)
        scale = ref.scale_f32(got_s * got_s, 4500)
        assert scale[3] == 0 and (scale[good] > 0).all()
        snr, code = ref.harmonic_ref(spec.cpu().numpy()[:, :n // 2], scale, 5, 1, 32)
        s = cells.snr.cpu().numpy()
        assert same_bits(s, snr) and np.array_equal(cells.code.cpu().numpy(), code)
        assert (s[3] == -1.0).all()
        again = be.harmonic_snr(plane, nharm=16, cell=32, nfft=nfft, stat_block=500, spectrum=spec)
        assert same_bits(again.snr.cpu().numpy(), snr)


def pulse_train(seed=0):
    """5 trials x 40 000 samples of N(0, 1) noise and a train of boxcar pulses
    of period 100.37 samples: 2 samples wide with amplitude 1.0 in trial 2, 4
    samples wide with amplitude 0.5 in trials 1 and 3."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((5, 40000)).astype(np.float32)
    for i in range(int(40000 / 100.37) + 1):
        t = int(round(i * 100.37))
        x[2, t:t + 2] += np.float32(1.0)
        x[1, t:t + 4] += np.float32(0.5)
        x[3, t:t + 4] += np.float32(0.5)
    return x


def test_synthetic_pulse_train(hip_lib):
    """A pulse train of period 100.37 samples in 5 x 40 000 samples of unit
    noise, threshold 15: the restatement on NumPy's float64 spectrum gives over
    the seeds 0 .. 3 a best z of 39.6 - 47.8 at trial 2 with 16 harmonics and
    the fundamental at 398.5 bins (true: 40000 / 100.37 = 398.525), while the
    noise-only trials top out at 8.3 - 11.1.  Asserted here: the first
    candidate is at trial 2 with 16 harmonics within half a bin of the true
    frequency, no candidate lies in trials 0 and 4, and the whole table equals
    the restatement's on the spectrum and the statistics of the device."""
    x = pulse_train()
    be = kh.backend()
    plane = _plane(x, dms=np.arange(5) * 2.0)
    got = be.periodicity_search(plane, threshold=15)
    print(got.array)
    assert len(got) >= 1 and got.cells.nfft == 40000 and got.cells.df == 0.25
    first = got[0]
    assert first["dm_index"] == 2 and first["nharm"] == 16 and first["dm"] == 4.0
    assert abs(first["freq"] / got.cells.df - 40000 / 100.37) <= 0.5
    assert first["period"] == 1.0 / first["freq"] and first["log_fap"] < -100
    assert not np.isin(got.dm_index, (0, 4)).any()
    spec = be.dm_spectrum(plane, mean=got.cells.mean).cpu().numpy()[:, :20000]
    std = got.cells.std.cpu().numpy()
    want, snr, code = ref.search_ref(spec, ref.scale_f32(std * std, 40000), 15.0, 5, 1, 32)
    print("restatement:", want)
    assert same_bits(got.cells.snr.cpu().numpy(), snr) and np.array_equal(got.cells.code.cpu().numpy(), code)
    rows = [(float(c["snr"]), int(c["dm_index"]), int(c["bin"]), int(c["nharm"]), int(c["ncells"])) for c in got.array]
    assert rows == want
    noise = snr[[0, 4]]
    print("best z", want[0][0], "noise-only trials top out at", noise.max())
    assert noise.max() < 15 < want[0][0]
    with pytest.raises(ValueError, match="threshold 1 exceed max_cells 10"):
        be.periodicity_search(plane, threshold=1.0, max_cells=10)


def test_api_end_to_end_pulsar(hip_lib):
    """make_pulses -> ISM.disperse(30) -> dedisperse -> periodicity_search: the
    set-up of tests/test_gpu_pulse_search.py::test_api_end_to_end_pulsar (64
    channels, 10 kHz, P = 50 ms, DM 30, 1.6384 s, 13 trial DMs 0 .. 60; T =
    15 635, nfft = 15 552, df = 0.643 Hz, 20 Hz = bin 31.1).

    The simulated pulsar has no radiometer noise: between the pulses the series
    is all but zero, and the only "noise" is the pulses' own.  With the default
    ``stat_block`` of 1024 samples (two periods) every block holds pulses, the
    block medians measure the pulsar itself -- std 17.4 at the true DM where
    the pulses are sharp, 9.7 three trials away where they are smeared -- and
    the normalisation flattens the DM response: the restatement on the CPU
    oracle's signal (oracle/pss_cpu.py, seeds 0 .. 11) then gives the
    fundamental alone (nharm 1, 19.93 Hz) at z = 5189 - 5281 in trial 9, 10 or
    3, the runner-up trial within 1.2 %, and trial 6 far behind.  That is the
    normalisation's doing, not the sum's.  With ``stat_block=128`` (12.8 ms, a
    quarter of the period and well inside its off-pulse stretch; the pulse's
    FWHM is 5.9 ms) the median block holds no pulse, as the block medians are
    meant to be used, and over the same 12 seeds the best candidate is always
    at DM index 6 with nharm 2 at 19.93 Hz (bin 62 / 2; |f - 20 Hz| = 0.067 Hz
    = 0.10 df), z = 3.0e6 - 5.1e6 (the off-pulse std is 0.43 - 0.56), 318 - 356
    candidates above 10; the runner-up trial is 5 or 7 with a best z of 0.094 -
    0.179 of trial 6's.  The device draws from another generator, so asserted
    is only: the strongest candidate is at DM index 6 within df of 20 Hz, and
    no other trial reaches half its z."""
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar
    from psrsigsim_amd.ism import ISM
    pss.seed(20250101)
    sig = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False)
    Pulsar(0.05, 1.0).make_pulses(sig, tobs=1.6384)
    ISM().disperse(sig, 30)
    be = kh.backend()
    plane = be.dedisperse(sig, np.arange(0, 65, 5))
    got = be.periodicity_search(plane, stat_block=128)
    per_trial = got.cells.snr.max(dim=1).values.cpu().numpy()
    order = np.argsort(-per_trial)
    print("candidates", len(got), "best", got[0], "std", got.cells.std.cpu().numpy())
    print("best z per trial", per_trial, "runner-up trial", order[1], per_trial[order[1]] / per_trial[order[0]])
    assert got.cells.nfft == 15552 and got.cells.df == 1e4 / 15552
    assert got[0]["dm_index"] == 6 and got[0]["dm"] == 30.0
    assert abs(got[0]["freq"] - 20.0) <= got.cells.df
    assert order[0] == 6 and per_trial[order[1]] <= 0.5 * per_trial[6]
