"""Host side of the acceleration search (no GPU): the exact table entry
``Backend.accel_shift_step``, the grid ``Backend.accel_trials``, the C ABI's
argument checks, which precede any launch, the properties of the definition
(tests/accel_ref.py) that the kernel's bounds rest on, and the CPU study that
motivates the stage: an accelerated pulse train is found at its own trial
acceleration and lost at zero."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from psrsigsim_amd import _lib
from tests import accel_ref as ref
from tests import periodicity_ref as pref
from tests.kernel_harness import check_rejections, host_pointer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 299792458.0


def _Backend():
    from psrsigsim_amd.telescope import Backend
    return Backend


# ---------------------------------------------------------------------------
# the table entry and the grid
# ---------------------------------------------------------------------------
def test_shift_step_is_the_exact_rounding():
    B = _Backend()
    for a, fs_MHz, T in ((1.0, 0.01, 65536), (-1.0, 0.01, 65536), (273.5, 0.0123, 1000), (-1e-3, 1.0, 1 << 20),
                         (5.0e-7, 3.3e-3, 7)):
        al = -Fraction(a) / (2 * Fraction(C) * Fraction(fs_MHz * 1e6))
        q = abs(al) * (1 << 64) + Fraction(1, 2)
        want = (q.numerator // q.denominator) * (1 if al >= 0 else -1)
        got = B.accel_shift_step(a, fs_MHz, T)
        assert isinstance(got, int) and got == want == ref.kappa_of_accel(a, fs_MHz)
        # positive is away from the observer: the series is read earlier, kappa < 0
        assert (got < 0) == (a > 0)
    assert B.accel_shift_step(0.0, 0.01, 1000) == 0
    assert B.accel_shift_step(-0.0, 0.01, 1000) == 0


def test_shift_step_limit():
    """|alpha| T = 1/2 exactly is accepted, anything beyond raises."""
    B = _Backend()
    # fs = 2^k / c would not be a float; build the limit from the other side:
    # a = c fs / T with fs 1e6 = 2^20 Hz and T = 2^10 -> alpha = 1 / (2 T) exactly
    fs_MHz = float(1 << 20) / 1e6
    assert fs_MHz * 1e6 == float(1 << 20)
    T = 1 << 10
    a = C * 1024.0                                       # c fs / T, exact in float64 (c < 2^29)
    assert Fraction(a) == Fraction(C) * 1024
    assert abs(ref.alpha_of_accel(a, fs_MHz)) * T == Fraction(1, 2)
    assert B.accel_shift_step(a, fs_MHz, T) == -((1 << 63) // T)
    assert B.accel_shift_step(-a, fs_MHz, T) == (1 << 63) // T
    with pytest.raises(ValueError, match="1/2"):
        B.accel_shift_step(np.nextafter(a, np.inf), fs_MHz, T)
    with pytest.raises(ValueError, match="1/2"):
        B.accel_shift_step(a, fs_MHz, T + 1)
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError, match="not finite"):
            B.accel_shift_step(bad, fs_MHz, T)
    with pytest.raises(ValueError):
        B.accel_shift_step(1.0, 0.0, T)
    with pytest.raises(ValueError):
        B.accel_shift_step(1.0, fs_MHz, 0)


def test_accel_trials_grid():
    B = _Backend()
    T, fs_MHz = 65536, 0.01
    for amax, tol in ((100.0, 1.0), (30000.0, 0.5), (0.0, 1.0), (5584.0, 1.0), (5585.0, 1.0)):
        g = B.accel_trials(T, fs_MHz, amax, tol)
        da = 8.0 * C * (fs_MHz * 1e6) * tol / (float(T) * float(T))
        n = int(np.ceil(amax / da))
        assert g.dtype == np.float64 and g.size == 2 * n + 1
        assert g[n] == 0.0 and np.array_equal(g, -g[::-1])
        assert np.array_equal(g, np.arange(-n, n + 1) * da) and np.all(np.diff(g) > 0)
        assert g[-1] >= amax and (n == 0 or g[-1] - da < amax)
        if n:
            # neighbours differ by tol samples at mid-observation: alpha T^2 / 4
            s = [float(ref.alpha_of_accel(a, fs_MHz)) * T * T / 4 for a in g[n:n + 2]]
            assert abs((s[0] - s[1]) - tol) < 1e-9
    for kw in (dict(amax=-1.0), dict(amax=np.nan), dict(tol=0.0), dict(tol=np.inf)):
        args = dict(amax=10.0, tol=1.0)
        args.update(kw)
        with pytest.raises(ValueError):
            B.accel_trials(T, fs_MHz, **args)


def test_python_level_rejections_touch_no_device():
    from psrsigsim_amd.telescope import DedispersedPlane

    class Stub(object):
        shape = (3, 4096)

        def __getattr__(self, name):
            raise AssertionError("the device buffer was touched (%s)" % name)

    B = _Backend()
    be = B(samprate=0.01)
    plane = DedispersedPlane(Stub(), np.arange(3.0), None, 0.01, 1400.0, 0)
    with pytest.raises(ValueError, match="either accels or amax"):
        be.accel_search(plane)
    with pytest.raises(ValueError, match="either accels or amax"):
        be.accel_search(plane, accels=[0.0], amax=1.0)
    for bad in ([], [np.nan], [[0.0, 1.0]], [0.0, np.inf]):
        with pytest.raises(ValueError, match="accels"):
            be.accel_snr(plane, bad)
    with pytest.raises(ValueError, match="1/2"):
        be.accel_snr(plane, [0.0, 2.0 * C * 1e4 / 4096])
    with pytest.raises(ValueError, match="nharm"):
        be.accel_snr(plane, [0.0], nharm=3)
    with pytest.raises(ValueError, match="max_bytes"):
        be.accel_snr(plane, [0.0], max_bytes=4096 * 4)
    with pytest.raises(ValueError, match="DedispersedPlane"):
        be.accel_resample(np.zeros((2, 8)), [0.0])


# ---------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_hashed():
    from psrsigsim_amd import build
    with open(os.path.join(ROOT, "include", "pss_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+pss_accel_resample\s*\(", header)
    assert "pss_accel_resample" in _lib.EXPORTS and len(_lib.EXPORTS["pss_accel_resample"][1]) == 12
    assert hasattr(_lib.load(), "pss_accel_resample")
    assert "pss_accel.hip" in build.UNITS
    assert any(os.path.basename(d) == "pss_accel.hip" for d in build.DEPS)           # source_hash() covers it


def test_entry_point_validates_arguments():
    """Every PSS_EINVAL of pss_accel_resample with NULL or host pointers: the
    checks precede any launch (no GPU touched)."""
    p = host_pointer()
    good = dict(x=p, nser=2, T=16, ld=16, src=p, kappa=p, sub=None, nrows=3, n_out=16, out=p, out_ld=16)
    big = (1 << 31) - 1
    check_rejections(_lib.load().pss_accel_resample, good,
                   ((dict(x=None), "x is NULL"), (dict(src=None), "src is NULL"), (dict(kappa=None), "kappa is NULL"),
                    (dict(out=None), "out is NULL"), (dict(nser=0), "nser 0 < 1"), (dict(nrows=0), "nrows 0 < 1"),
                    (dict(nrows=-2), "nrows -2 < 1"), (dict(T=0, ld=0), "T 0 < 1"),
                    (dict(T=1 << 31, ld=1 << 31), "T 2147483648 > 2^31 - 1"), (dict(ld=15), "ld 15 < T 16"),
                    (dict(n_out=0), "n_out 0 < 1"), (dict(n_out=17, out_ld=17), "n_out 17 > T 16"),
                    (dict(out_ld=15), "out_ld 15 < n_out 16"),
                    (dict(T=big, ld=big, n_out=big, out_ld=big, nrows=1 << 14),
                     "1048576 time tiles x 2048 row groups exceed 2^31 - 1 workgroups")), prefix="accel_resample: ")


# ---------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------
def test_definition_is_monotone_with_fixed_ends():
    """For random (T, kappa), T <= 5000, the whole int64 range of kappa
    included: once K is clamped to 2^63 // T the index is non-decreasing, steps
    by 0, 1 or 2, starts at 0, ends at T - 1, and the index clamp never acts."""
    rng = np.random.default_rng(11)
    cases = [(1, 0), (1, -(1 << 63)), (2, (1 << 63) - 1), (3, (1 << 63) // 3), (5000, -(1 << 63)), (4999, 1 << 62)]
    for _ in range(60):
        T = int(rng.integers(1, 5001))
        kmax = (1 << 63) // T
        pick = rng.integers(0, 4)
        k = (int(rng.integers(-kmax, kmax + 1)), int(rng.integers(-(1 << 63), (1 << 63) - 1, endpoint=True)),
             kmax * int(rng.choice([-1, 1])), int(rng.integers(-1000, 1001)) * (kmax // 1000))[pick]
        cases.append((T, k))
    twos = zeros = 0
    for T, k in cases:
        raw = ref.index_unclamped(T, k)
        idx = ref.index(T, k)
        assert np.array_equal(raw, idx), (T, k)                     # the clamp is inactive
        assert idx[0] == 0 and idx[-1] == T - 1, (T, k)
        d = np.diff(idx)
        assert d.size == 0 or (d.min() >= 0 and d.max() <= 2), (T, k)
        twos += int((d == 2).sum())
        zeros += int((d == 0).sum())
        K, sg = ref.clamp_step(k, T)
        assert K <= (1 << 63) // T and sg in (-1, 1)
        # cutting the output short does not change the map
        n = max(1, T // 3)
        assert np.array_equal(ref.index(T, k, n), idx[:n])
    assert twos > 100 and zeros > 100
    # the mid-observation shift of kappa_of_shift is s_max
    for T, s in ((65536, 96), (65536, -192), (1001, 7)):
        idx = ref.index(T, ref.kappa_of_shift(s, T))
        assert idx[T // 2] - T // 2 == s


def test_unclamped_step_would_leave_the_row():
    """What the clamp of K is for: without it the map overshoots the row."""
    T = 1000
    K = 4 * ((1 << 63) // T)
    raw = np.arange(T) + np.array(ref.shift(T, K), dtype=np.int64)
    assert raw.max() > T - 1 and np.diff(raw).min() < 0


# ---------------------------------------------------------------------------
# the study: what the stage is for
# ---------------------------------------------------------------------------
def study_series(seed=0):
    return ref.accel_signal(T=65536, period=128.37, s_max=96, amp=0.6, width=0.02, seed=seed)


def test_accelerated_pulsar_is_found_at_its_own_trial():
    """x = N(0, 1) + 0.6 exp(-(d / 0.02)^2 / 2) at P = 128.37 samples with a
    mid-observation shift of 96 samples in T = 65536, seed 0; trials s_max =
    -192, -144 .. 192; 16 harmonics, cells of 32 bins.  The true trial reaches
    z = 76.9 with bin 4084 at 8 harmonics (a fundamental of 510.5 bins =
    65536 / 128.37), zero acceleration 15.4, the best other trial 24.5."""
    T = 65536
    x = study_series(0)
    mean = np.float32(x.astype(np.float64).mean())
    scale = pref.scale_f32(x.astype(np.float64).var(), T)
    trials = list(range(-192, 193, 48))
    best = {}
    for s in trials:
        y = ref.resample(x[None, :], [0], [ref.kappa_of_shift(s, T)], sub=[mean])[0]
        spec = np.fft.rfft(y.astype(np.float64)).astype(np.complex64)[None, :T // 2]
        snr, code = pref.harmonic_ref(spec, scale, 5, 1, 32)
        q = int(np.argmax(snr[0]))
        k, lev = pref.decode(code, 32)
        best[s] = (float(snr[0, q]), int(k[0, q]), int(lev[0, q]))
    print(best)
    top = max(trials, key=lambda s: best[s][0])
    assert top == 96
    assert best[96][1:] == (4084, 3)
    others = max(best[s][0] for s in trials if s != 96)
    assert best[96][0] >= 2.0 * others, (best[96][0], others)
    assert abs(best[96][0] - 76.9) < 0.1 and abs(others - 24.5) < 0.1


# ---------------------------------------------------------------------------
# the kernel's tile and window logic, ported
# ---------------------------------------------------------------------------
def _tile_constants():
    """(TB, NR, WIN) read from csrc/pss_accel.hip."""
    with open(os.path.join(ROOT, "psrsigsim_amd", "csrc", "pss_accel.hip")) as f:
        src = f.read()
    runs = int(re.search(r"#define PSS_ACCEL_RUNS (\d+)", src).group(1))
    threads = int(re.search(r"kAcThreads = (\d+);", src).group(1))
    run = int(re.search(r"kAcRun = (\d+);", src).group(1))
    nr = int(re.search(r"kAcNR = (\d+);", src).group(1))
    assert re.search(r"kAcWin = 2 \* kAcTB;", src) and re.search(r"kAcTB = kAcThreads \* kAcRun \* kAcRuns;", src)
    tb = threads * run * runs
    return tb, nr, 2 * tb, run


def port_resample(x, ld_pad, base, src, kap, n_out, TB, NR, WIN, RUN):
    """k_accel_resample step by step in Python integers (sub == NULL): per
    (tile, group) the rows' source ranges, the window and which rows it
    serves, the staging (16-B groups inside the row, element loads at its
    ends), and per run of RUN outputs the shift at the two ends.  Asserts every
    bound the kernel relies on; ``base`` is the float offset of x in memory
    modulo 4.  Returns (out, outputs staged, outputs direct)."""
    nser, T = x.shape
    ld = T + ld_pad
    nrows = len(src)

    def sh(t, K):
        return (t * (T - t) * K + (1 << 63)) >> 64

    def idx(t, K, sg):
        return min(max(t + sg * sh(t, K), 0), T - 1)

    out = np.full((nrows, n_out), np.nan, dtype=np.float32)
    nst = ndir = 0
    for t0 in range(0, n_out, TB):
        ln = min(TB, n_out - t0)
        for r0 in range(0, nrows, NR):
            nr = min(NR, nrows - r0)
            rows = [r0 + min(j, nr - 1) for j in range(NR)]          # a ragged group repeats its last row
            Ks = [ref.clamp_step(kap[r], T) for r in rows]
            si = [min(max(int(src[r]), 0), nser - 1) for r in rows]
            lo = [idx(t0, K, sg) for K, sg in Ks]
            hi = [idx(t0 + ln - 1, K, sg) for K, sg in Ks]
            assert all(l <= h for l, h in zip(lo, hi))
            wlo = min(l for l, s in zip(lo, si) if s == si[0])
            wb = wlo - ((base + si[0] * ld + wlo) & 3)
            staged = [s == si[0] and h - wb < WIN for s, h in zip(si, hi)]
            need = max([h - wb + 1 for h, st in zip(hi, staged) if st] + [0])
            win = None
            if need:
                assert 1 <= need <= WIN and wb >= -3 and wb + need <= T
                nq = (need + 3) >> 2
                assert 4 * nq <= WIN
                win = np.zeros(WIN, dtype=np.float32)
                if wb >= 0 and wb + 4 * nq <= T:
                    win[:4 * nq] = x[si[0], wb:wb + 4 * nq]
                else:
                    for p in range(4 * nq):
                        if 0 <= wb + p < T:
                            win[p] = x[si[0], wb + p]
            for j in range(nr):
                K, sg = Ks[j]
                for tl in range(0, ln, RUN):
                    nv = min(RUN, ln - tl)
                    t, tb = t0 + tl, t0 + tl + nv - 1
                    sa, se = sh(t, K), sh(tb, K)
                    copy = (2 * tb <= T or 2 * t >= T) and sa == se
                    for e in range(nv):
                        i = min(max(t + e + sg * sa, 0), T - 1) if copy else idx(t + e, K, sg)
                        if staged[j]:
                            assert 0 <= i - wb < need
                            out[r0 + j, t + e] = win[i - wb]
                            nst += 1
                        else:
                            assert 0 <= i < T
                            out[r0 + j, t + e] = x[si[j], i]
                            ndir += 1
    return out, nst, ndir


def test_kernel_port_stays_in_bounds_and_gives_the_definition():
    """The port of the kernel's integer logic against the definition for
    random shapes: tables over the whole int64 range, clamped and mixed src,
    every alignment, ragged tiles and groups -- both routes taken, every LDS
    and global index inside its bounds, the bits the definition's."""
    TB, NR, WIN, RUN = _tile_constants()
    assert (TB, NR, WIN, RUN) == (2048, 8, 4096, 4)
    rng = np.random.default_rng(1)
    tot_st = tot_dir = 0
    for trial in range(30):
        T = int(rng.integers(1, 3 * TB))
        n_out = int(rng.integers(1, T + 1))
        nser = int(rng.integers(1, 4))
        nrows = int(rng.integers(1, 2 * NR + 3))
        kmax = (1 << 63) // T
        mode = trial % 3
        kap = []
        for r in range(nrows):
            if mode == 0:
                k = int(rng.integers(-kmax, kmax, endpoint=True))
            elif mode == 1:
                k = ref.kappa_of_shift(int(rng.integers(-8, 9)), T) if T > 64 else 0
            else:
                k = [-(1 << 63), (1 << 63) - 1, kmax, kmax + 1, 0, -kmax][int(rng.integers(0, 6))]
            kap.append(max(min(k, (1 << 63) - 1), -(1 << 63)))
        src = rng.integers(-1, nser + 1, nrows) if trial % 2 else np.repeat(rng.integers(0, nser), nrows)
        x = rng.standard_normal((nser, T)).astype(np.float32)
        got, nst, ndir = port_resample(x, int(rng.integers(0, 7)), int(rng.integers(0, 4)), src, kap, n_out,
                                       TB, NR, WIN, RUN)
        want = ref.resample(x, src, kap, None, n_out)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), trial
        tot_st += nst
        tot_dir += ndir
    assert tot_st > 10000 and tot_dir > 10000
