"""The acceleration resampler on the GPU (``pss_accel_resample``,
``Backend.accel_resample`` / ``accel_snr`` / ``accel_search``).

The oracle is tests/accel_ref.py: Python integers for the index, NumPy float32
for the one subtraction.  The kernel moves bits, so every comparison is
``array_equal`` on the uint32 view -- no tolerance, no excluded sample.

Every kernel-level case gives the kernel views inside larger tensors: row
strides ld > T and out_ld > n_out, every float offset of input and output.
The input's parent holds 2^20 around and behind the rows, two whole guard rows
before the first and after the last series included, so that an unclamped
``src`` or index reads allocated memory and breaks the equality; the output's
parent holds a sentinel that is checked untouched afterwards.  The data are
seeded normal float32 with a -0.0 and a denormal.

The kernel's tile (pss_accel.hip): a workgroup owns TB = 2048 output times of
NR = 8 consecutive rows; the rows that read the series of the group's first row
and whose source range ends inside the window of WIN = 4096 floats (from the
lowest source index among them, moved down to the 16-B grid of the address) are
gathered from LDS, every other row from global memory.
"""
import numpy as np
import pytest

from tests import accel_ref as ref
from tests import kernel_harness as kh
from tests.kernel_harness import same_bits

pytestmark = pytest.mark.gpu

TB, NR, WIN = 2048, 8, 4096
IN_GUARD = float(1 << 20)
OUT_GUARD = -7.0
GUARD_ROWS = 2
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def data(nser, T, seed):
    x = np.random.default_rng(seed).standard_normal((nser, T)).astype(np.float32)
    x[0, 0] = -0.0
    if T > 2:
        x[0, 2] = x[nser - 1, 2] = np.float32(1e-40)      # a denormal
        assert 0 < x[nser - 1, 2] < np.finfo(np.float32).tiny
    return x


def _case(name):
    """(x [nser][T], src, kappa, sub or None, n_out) of the issue's cases."""
    if name == "copy1":
        return data(1, 1, 1), [0], [0], None, 1
    if name == "copy64":
        return data(1, 64, 2), [0], [0], None, 64
    if name in ("odd", "odd777"):
        # 5 rows of both signs, src not monotone, one below 0 and one >= nser
        T = 1000
        kap = [ref.kappa_of_shift(s, T) for s in (37, -11, 0, -100, 125)]
        return data(3, T, 3), [2, -1, 1, 3, 0], kap, None, (T if name == "odd" else 777)
    if name == "limit":
        T = 1000
        kmax = (1 << 63) // T
        kap = [kmax, -kmax, kmax + 1, -(kmax + 1), I64_MIN, I64_MAX]
        d = np.diff(ref.index(T, kmax))
        assert (d == 0).any() and (d == 2).any() and np.array_equal(ref.index(T, I64_MAX), ref.index(T, kmax))
        return data(2, T, 4), [0, 1, 1, 0, 1, 0], kap, None, T
    if name in ("tiles9", "tiles17"):
        # TB + 1 is two tiles, 9 rows a full group and one: 4 workgroups;
        # 3 TB + 5 with 17 rows is 4 x 3 = 12 (XCD runs of unequal length)
        T, rows = (TB + 1, 9) if name == "tiles9" else (3 * TB + 5, 17)
        kap = [ref.kappa_of_shift(s, T) for s in np.linspace(-64, 64, rows).round().astype(int)]
        return data(3, T, 5), [r // 8 for r in range(rows)], kap, None, T
    if name == "smax0_7":
        T = 3 * TB + 5
        return data(1, T, 6), [0] * 8, [ref.kappa_of_shift(s, T) for s in range(8)], None, T
    if name == "mixed":
        T = 2 * TB + 77
        kap = [ref.kappa_of_shift(s, T) for s in (5, -5, 300, 0, -300, 1, 2, 3)]
        return data(3, T, 7), [0, 1, 0, 1, 2, 0, 0, 1], kap, None, T
    if name == "sub":
        T = 2500
        kap = [ref.kappa_of_shift(s, T) for s in (0, 9, -9, 0)]
        x = data(2, T, 8)
        return x, [0, 1, 0, 1], kap, np.array([0.0, 1.5, -3.25e-3, x[1, 5]], dtype=np.float32), T
    if name == "hi":
        # T above 2^20: the high word of the product, near the limit and far from it
        T = (1 << 20) + 3
        kmax = (1 << 63) // T
        return data(1, T, 9), [0, 0, 0, 0], [kmax - 5, -(kmax - 5), ref.kappa_of_shift(3, T), 0], None, T
    raise KeyError(name)


@kh.once
def reference(name):
    """A case and its oracle, computed once and shared (read-only)."""
    x, src, kap, sub, n_out = _case(name)
    return x, src, kap, sub, n_out, ref.resample(x, src, kap, sub, n_out)


def run_kernel(hip_lib, x, src, kappa, sub, n_out, ld=None, out_ld=None, in_off=0, out_off=0, want_ptr=False):
    """pss_accel_resample on views inside larger tensors (tests/kernel_harness.py):
    ``x`` with row stride ld between guards that include GUARD_ROWS whole rows
    on either side, ``out`` with row stride out_ld.  Returns out
    [nrows][n_out] after checking that nothing outside out[r][0 .. n_out) was
    written."""
    import torch
    from psrsigsim_amd import _lib
    nser, T = x.shape
    nrows = len(src)
    ld = T + 5 if ld is None else ld
    out_ld = (n_out + 7) // 4 * 4 if out_ld is None else out_ld
    assert ld > T and out_ld > n_out
    xin = kh.GuardedInput(x, ld, in_off, IN_GUARD, guard_rows=GUARD_ROWS)
    out = kh.GuardedOutput(nrows, n_out, out_ld, out_off, OUT_GUARD)
    src_d = torch.from_numpy(np.array(src, dtype=np.int32)).cuda()
    kap_d = torch.from_numpy(np.array(kappa, dtype=np.int64)).cuda()
    sub_d = None if sub is None else torch.from_numpy(np.array(sub, dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    rc = hip_lib.pss_accel_resample(xin.ptr, nser, T, ld, src_d.data_ptr(), kap_d.data_ptr(),
                                    None if sub_d is None else sub_d.data_ptr(), nrows, n_out, out.ptr, out_ld, None)
    _lib.check(rc, "accel_resample")
    torch.cuda.synchronize()
    got = out.read()
    return (got, xin.ptr) if want_ptr else got


def routes(ptr, ld, nser, T, n_out, src, kappa):
    """The kernel's rule restated: {(tile, group): [staged?] per row}."""
    def idx(t, k):
        K, sg = ref.clamp_step(k, T)
        return min(max(t + sg * ref.shift(T, K, [t])[0], 0), T - 1)
    out = {}
    for ti, t0 in enumerate(range(0, n_out, TB)):
        ln = min(TB, n_out - t0)
        for g, r0 in enumerate(range(0, len(src), NR)):
            rows = list(range(r0, min(r0 + NR, len(src))))
            si = [min(max(int(src[r]), 0), nser - 1) for r in rows]
            lo = [idx(t0, kappa[r]) for r in rows]
            hi = [idx(t0 + ln - 1, kappa[r]) for r in rows]
            wlo = min(l for l, s in zip(lo, si) if s == si[0])
            wb = wlo - ((ptr // 4 + si[0] * ld + wlo) & 3)
            out[(ti, g)] = [s == si[0] and h - wb < WIN for s, h in zip(si, hi)]
    return out


# ---------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["copy1", "copy64", "odd", "odd777", "limit", "tiles9", "tiles17", "smax0_7",
                                  "mixed", "sub", "hi"])
def test_kernel_moves_the_bits_of_the_definition(hip_lib, name):
    x, src, kap, sub, n_out, want = reference(name)
    assert same_bits(run_kernel(hip_lib, x, src, kap, sub, n_out), want)


@pytest.mark.parametrize("in_off,out_off,ld_pad,out_pad", [(0, 0, 8, 4), (1, 3, 5, 3), (2, 2, 6, 1), (3, 1, 7, 2),
                                                           (0, 2, 4, 4), (2, 0, 1, 8)])
@pytest.mark.parametrize("name", ["odd", "odd777", "mixed"])
def test_alignment_and_pitch_do_not_matter(hip_lib, name, in_off, out_off, ld_pad, out_pad):
    x, src, kap, sub, n_out, want = reference(name)
    got = run_kernel(hip_lib, x, src, kap, sub, n_out, ld=x.shape[1] + ld_pad, out_ld=n_out + out_pad,
                     in_off=in_off, out_off=out_off)
    assert same_bits(got, want)


def test_sub_is_one_float32_subtraction_and_null_copies(hip_lib):
    x, src, kap, sub, n_out, want = reference("sub")
    got = run_kernel(hip_lib, x, src, kap, sub, n_out)
    assert same_bits(got, want)
    # x - x = +0.0 somewhere in row 3, the denormal minus 0.0 stays a denormal
    idx3 = ref.index(x.shape[1], kap[3])
    assert got[3][np.flatnonzero(idx3 == 5)[0]] == 0.0
    assert same_bits(got[0][2:3], x[0][2:3] - np.float32(0.0))
    copy = run_kernel(hip_lib, x, src, kap, None, n_out)
    assert same_bits(copy, ref.resample(x, src, kap, None, n_out))
    assert np.signbit(copy[0, 0]) and copy[0, 0] == 0.0                      # -0.0 stays -0.0
    assert same_bits(copy[3][2:3], np.array([1e-40], dtype=np.float32))      # and the denormal


def test_routes_give_the_same_bits(hip_lib):
    """One series, 8 rows, the last tile cut so that row 0's source range ends
    one sample inside the window that row 1 (a large negative shift) opens --
    staged -- and one sample past it -- direct."""
    T = 40000
    kmax = (1 << 63) // T
    src = [0] * 8
    kap = [0, -(kmax * 4 // 5)] + [ref.kappa_of_shift(s, T) for s in (1, -2, 3, -4, 5, -6)]
    x = data(1, T, 21)
    t0 = 5 * TB
    # find the cut with the pointer of a first run (the parent's layout is the same every time)
    got, ptr = run_kernel(hip_lib, x, src, kap, None, t0 + 1, want_ptr=True)
    assert same_bits(got, ref.resample(x, src, kap, None, t0 + 1))
    K1, sg1 = ref.clamp_step(kap[1], T)
    wlo = t0 - ref.shift(T, K1, [t0])[0]
    wb = wlo - ((ptr // 4 + wlo) & 3)
    ln = WIN - (t0 - wb)                                  # t0 + ln - 1 - wb = WIN - 1
    assert 1 <= ln < TB
    for n_out, row0_staged in ((t0 + ln, True), (t0 + ln + 1, False)):
        got, p2 = run_kernel(hip_lib, x, src, kap, None, n_out, want_ptr=True)
        assert p2 % 16 == ptr % 16
        r = routes(p2, T + 5, 1, T, n_out, src, kap)
        assert r[(5, 0)][0] is row0_staged and r[(5, 0)][1] is True
        flat = [v for m in r.values() for v in m]
        assert any(flat) and not all(flat)                # both routes are taken
        assert same_bits(got, ref.resample(x, src, kap, None, n_out))
    # the mixed group: rows of another series than the first row's go direct
    x, src, kap, sub, n_out, want = reference("mixed")
    got, ptr = run_kernel(hip_lib, x, src, kap, None, n_out, want_ptr=True)
    r = routes(ptr, x.shape[1] + 5, 3, x.shape[1], n_out, src, kap)
    assert r[(0, 0)] == [True, False, True, False, False, True, True, False]
    assert same_bits(got, want)


def test_rows_are_independent(hip_lib):
    """A row's bits depend on neither its position, its neighbours (and so its
    route) nor the alignment."""
    T = TB + 300
    x = data(3, T, 22)
    k = ref.kappa_of_shift(-41, T)
    sub = np.float32(0.375)
    want = ref.resample(x, [1], [k], [sub])[0]
    alone = run_kernel(hip_lib, x, [1], [k], [sub], T)
    assert same_bits(alone[0], want)
    # row 3 of a group led by another series (direct), then by its own (staged)
    for lead in (0, 1):
        src = [lead, 2, 0, 1, 1, 2, 0, 1, 1]
        kap = [ref.kappa_of_shift(s, T) for s in (3, -7, 100, 0, 50, 0, -3, 9, 0)]
        kap[3] = kap[8] = k
        subs = np.arange(9, dtype=np.float32)
        subs[3] = subs[8] = sub
        for in_off, out_off in ((0, 0), (3, 1)):
            got = run_kernel(hip_lib, x, src, kap, subs, T, in_off=in_off, out_off=out_off)
            assert same_bits(got[3], want) and same_bits(got[8], want)
            assert same_bits(got, ref.resample(x, src, kap, subs))


# ---------------------------------------------------------------------------
# the API
# ---------------------------------------------------------------------------
def _plane(x, samprate=0.01):
    import torch
    from psrsigsim_amd.telescope import DedispersedPlane
    x = np.asarray(x, dtype=np.float32)
    return DedispersedPlane(torch.from_numpy(np.array(x)).cuda(), np.arange(float(x.shape[0])),
                            np.zeros((x.shape[0], 1), dtype=np.int32), samprate, 1500.0, 0)


def _series(T):
    rng = np.random.default_rng(31)
    mean = rng.uniform(-50.0, 200.0, size=5)
    sigma = rng.uniform(0.5, 20.0, size=5)
    t = np.arange(T)
    x = mean[:, None] + sigma[:, None] * rng.standard_normal((5, T))
    x[2] += 1.5 * sigma[2] * (np.abs((t / 37.3) % 1.0) < 0.1)
    return x.astype(np.float32), mean, sigma


def test_api_resample(hip_lib):
    import torch
    from psrsigsim_amd.telescope import Backend
    be = kh.backend()
    T = 4500
    x, mean, sigma = _series(T)
    plane = _plane(x)
    m32 = mean.astype(np.float32)
    for n in (T, 1234):
        y = be.accel_resample(plane, [0.0], mean=mean, n_out=n)
        assert tuple(y.shape) == (5, 1, n) and y.data_ptr() % 16 == 0 and y.stride(1) % 4 == 0
        assert same_bits(y[:, 0].cpu().numpy(), x[:, :n] - m32[:, None])
    # the default mean is the block-median mean the other stages measure
    own = be.harmonic_snr(plane).mean.to(torch.float32)
    y = be.accel_resample(plane, [0.0])
    assert torch.equal(y[:, 0].contiguous().view(torch.int32), (plane.data - own[:, None]).view(torch.int32))
    # several accelerations, a range of trials: row (j, a) is the restatement's
    acc = Backend.accel_trials(T, 0.01, 3.0e7, tol=2.0)
    kap = [Backend.accel_shift_step(a, 0.01, T) for a in acc]
    assert acc.size >= 5 and kap == [ref.kappa_of_accel(a, 0.01) for a in acc]
    y = be.accel_resample(plane, acc, trials=(1, 4), mean=mean).cpu().numpy()
    assert y.shape == (3, acc.size, T)
    want = ref.resample(x, np.repeat([1, 2, 3], acc.size), kap * 3, np.repeat(m32[1:4], acc.size))
    assert same_bits(np.ascontiguousarray(y).reshape(-1, T), want)
    assert plane.data.cpu().numpy().tobytes() == x.tobytes()                 # the plane is left as it was


@pytest.mark.parametrize("T", [4500, 4374])
def test_api_snr_at_zero_is_the_periodicity_search(hip_lib, T):
    """accels = [0.0] gives the maps of harmonic_snr, with given and with
    measured statistics (4374 = 2 x 3^7 is a transform length off the 16-B
    grid)."""
    import torch
    be = kh.backend()
    x, mean, sigma = _series(T)
    plane = _plane(x)
    for kw in (dict(mean=mean, std=sigma, nharm=8, cell=64, fmin=3.0), dict(), dict(nharm=2, nfft=2 * T)):
        h = be.harmonic_snr(plane, **kw)
        a = be.accel_snr(plane, [0.0], **kw)
        assert torch.equal(a.snr.view(torch.int32), h.snr.view(torch.int32)) and torch.equal(a.code, h.code)
        assert torch.equal(a.bin, h.bin) and torch.equal(a.nharm_log2, h.nharm_log2) and torch.equal(a.freq, h.freq)
        assert a.acc_index.dtype == torch.int32 and a.acc_index.shape == a.snr.shape
        assert int(a.acc_index.abs().max()) == 0
        assert (a.nfft, a.nbin, a.kmin, a.cell, a.df) == (h.nfft, h.nbin, h.kmin, h.cell, h.df)
        assert np.array_equal(a.accels, [0.0])


def test_api_snr_chunking_and_ties(hip_lib):
    """The maps are independent of max_bytes (whole trials per chunk, one trial
    per chunk, blocks of accelerations of one trial), and a tie goes to the
    acceleration given first."""
    import torch
    from psrsigsim_amd.telescope import Backend
    be = kh.backend()
    T = 4500
    x, mean, sigma = _series(T)
    plane = _plane(x)
    acc = Backend.accel_trials(T, 0.01, 2.4e6, tol=1.0)[[3, 0, 2, 4, 1]]       # not sorted: order matters for ties
    assert acc.size == 5
    kw = dict(nharm=8, cell=64, fmin=3.0, mean=mean, std=sigma)
    full = be.accel_snr(plane, acc, **kw)
    assert int(full.acc_index.max()) > 0
    # each acceleration on its own, maximised on the host: first wins ties
    each = [be.accel_snr(plane, [a], **kw) for a in acc]
    s = np.stack([e.snr.cpu().numpy() for e in each])
    first = np.argmax(s, axis=0)                           # numpy: the first maximum
    assert np.array_equal(full.acc_index.cpu().numpy(), first)
    assert same_bits(full.snr.cpu().numpy(), np.take_along_axis(s, first[None], 0)[0])
    c = np.stack([e.code.cpu().numpy() for e in each])
    assert np.array_equal(full.code.cpu().numpy(), np.take_along_axis(c, first[None], 0)[0])
    nbin = T // 2
    per_row = T * 4 + (nbin + 1) * 8 + nbin * 4
    for mb in (per_row, 2 * per_row + 100, 5 * per_row, 7 * per_row, 11 * per_row):
        part = be.accel_snr(plane, acc, max_bytes=mb, **kw)
        assert torch.equal(part.snr.view(torch.int32), full.snr.view(torch.int32))
        assert torch.equal(part.code, full.code) and torch.equal(part.acc_index, full.acc_index)
    with pytest.raises(ValueError, match="max_bytes"):
        be.accel_snr(plane, acc, max_bytes=per_row - 1, **kw)
    # the given statistics and the tables go over the upload stream after a large run: the same maps
    from psrsigsim_amd import _engine
    mode = _engine.UPLOAD_MODE
    _engine.UPLOAD_MODE = "stream"
    try:
        up = be.accel_snr(plane, acc, **kw)
        y_up = be.accel_resample(plane, acc[:2], mean=mean)
    finally:
        _engine.UPLOAD_MODE = mode
    assert torch.equal(up.snr.view(torch.int32), full.snr.view(torch.int32))
    assert torch.equal(up.code, full.code) and torch.equal(up.acc_index, full.acc_index)
    assert torch.equal(up.mean, full.mean) and torch.equal(up.std, full.std)
    assert torch.equal(y_up.view(torch.int32), be.accel_resample(plane, acc[:2], mean=mean).view(torch.int32))
    two = be.accel_snr(plane, [acc[0], acc[0]], **kw)
    assert int(two.acc_index.abs().max()) == 0
    assert torch.equal(two.snr.view(torch.int32), each[0].snr.view(torch.int32)) and torch.equal(two.code, each[0].code)
    for mb in (per_row, 2 * per_row):
        two = be.accel_snr(plane, [acc[0], acc[0]], max_bytes=mb, **kw)
        assert int(two.acc_index.abs().max()) == 0


def test_api_end_to_end(hip_lib):
    """The accelerated pulse train of tests/test_accel_host.py (seed 0: P =
    128.37 samples, a mid-observation shift of 96 samples in 65536) as a
    one-trial plane.  The sample rate T^2 / (8 c) Hz makes one sample of shift
    1 m/s^2, so the truth is a = -96 m/s^2 and accel_trials(amax = 192, tol =
    48) is the grid -192, -144 .. 192 of the host study.  accel_search finds
    the pulsar at the true trial within a bin of 65536 / 128.37 = 510.52 bins,
    at least 1.5 times as strong as periodicity_search sees it (CPU ratio: 3.6
    to 6.5 over six seeds).

    Measured on an MI355X: accel_search snr 76.96 at acc_index 2 (-96 m/s^2),
    510.500 bins at 8 harmonics; periodicity_search snr 15.38 (ratio 5.0)."""
    from psrsigsim_amd.telescope import Backend
    T = 65536
    x = ref.accel_signal(T=T, period=128.37, s_max=96, amp=0.6, width=0.02, seed=0)
    fs_MHz = T * T / (8.0 * ref.C_M_S) / 1e6
    be = Backend(samprate=fs_MHz, name="B")
    plane = _plane(x[None, :], samprate=fs_MHz)
    grid = Backend.accel_trials(T, fs_MHz, 192.0, tol=48.0)
    assert grid.size == 9 and np.allclose(grid, np.arange(-192, 193, 48), rtol=1e-12, atol=0)
    true = int(np.argmin(np.abs(grid + 96.0)))
    assert true == 2
    assert abs(Backend.accel_shift_step(grid[true], fs_MHz, T) - ref.kappa_of_shift(96, T)) <= 1
    cand = be.accel_search(plane, amax=192.0, tol=48.0)
    plain = be.periodicity_search(plane, threshold=5.0)
    assert len(cand) >= 1 and len(plain) >= 1
    best = cand[0]
    bins = best["freq"] / cand.cells.df
    print("accel_search: snr %.2f, acc_index %d, accel %.3f, %.3f bins at %d harmonics; periodicity_search: snr %.2f"
          % (best["snr"], best["acc_index"], best["accel"], bins, best["nharm"], plain.snr[0]))
    assert best["acc_index"] == true and best["accel"] == grid[true]
    assert abs(bins - T / 128.37) <= 1.0
    assert best["snr"] >= 1.5 * plain.snr[0]
    assert best["snr"] == cand.snr.max() and np.all(np.diff(cand.snr) <= 0)
    assert int(cand.cells.acc_index.max()) < grid.size
