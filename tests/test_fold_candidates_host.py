"""Host side of the candidate fold (no GPU): the exact phase step, every
Python-level rejection of ``Backend._fold_plan`` (nothing reaches the device),
its DM bookkeeping and chunking, the C ABI's argument checks, which precede
any launch, and ``FoldedCandidates.refine`` on cubes built in NumPy against
the plain-loop restatement (tests/fold_ref.py)."""
import os
import re

import numpy as np
import pytest

from psrsigsim_amd import _lib
from tests import fold_ref as ref
from tests.kernel_harness import check_rejections, host_pointer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _Backend():
    from psrsigsim_amd.telescope import Backend
    return Backend


class _StubBuf(object):
    """Stands in for the signal's device buffer: nothing of it may be read."""

    def __getattr__(self, name):
        raise AssertionError("the device buffer was touched (%s)" % name)


def _signal(N=16384, fold=False, **kw):
    from psrsigsim_amd.signal import FilterBankSignal
    sig = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=fold, **kw)
    sig._buf = _StubBuf()
    sig._ncols = sig._nsamp = N
    return sig


# ---------------------------------------------------------------------------
# the phase step
# ---------------------------------------------------------------------------
def test_phase_step_pinned_values():
    B = _Backend()
    assert B._phase_step(100.37) == 183787427256247392 == ref.phase_step(100.37)
    assert B._phase_step(500.0) == 36893488147419103 == ref.phase_step(500.0)
    assert B._phase_step(64.0) == 1 << 58 == ref.phase_step(64.0)
    # period [s] x samprate [MHz]: 1e-6 MHz is one sample a second (1e-6 * 1e6 == 1.0 in float64)
    assert 1e-6 * 1e6 == 1.0
    assert B.fold_phase_step(100.37, 1e-6) == 183787427256247392
    assert B.fold_phase_step(500.0, 1e-6) == 36893488147419103
    assert B.fold_phase_step(64.0, 1e-6) == 1 << 58
    assert B.fold_phase_step(0.05, 0.01) == 36893488147419103           # 50 ms at 10 kHz: 500 samples
    assert isinstance(B.fold_phase_step(0.05, 0.01), int)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="period"):
            B._phase_step(bad)


def test_phase_step_limit_at_one_sample_per_bin():
    """inc nbin <= 2^64 holds exactly at Ps = nbin and fails just below it."""
    B = _Backend()
    for nbin in (2, 64, 1024):
        assert B._phase_step(float(nbin)) * nbin == 1 << 64
        assert B._phase_step(float(nbin)) == ref.inc_limit(nbin)
        assert B._phase_step(np.nextafter(float(nbin), 0.0)) * nbin > 1 << 64
        assert B._phase_step(np.nextafter(float(nbin), np.inf)) * nbin <= 1 << 64


def test_float_phase_disagrees_with_the_definition():
    """Why the phase is fixed point: at P = 100.37 samples, 64 bins and 40 000
    samples the float64 floor(frac(u / P) nbin) differs at a few samples."""
    u = np.arange(40000, dtype=np.float64)
    fl = np.floor(np.modf(u / 100.37)[0] * 64).astype(np.int64)
    ex = ref.bins(40000, ref.phase_step(100.37), 0, 64)
    assert 0 < int((fl != ex).sum()) < 20
    assert ex.min() == 0 and ex.max() == 63


# ---------------------------------------------------------------------------
# _fold_plan
# ---------------------------------------------------------------------------
def test_plan_rejections_never_reach_the_device(monkeypatch):
    from psrsigsim_amd import _engine
    from psrsigsim_amd.telescope import PeriodCandidates
    from psrsigsim_amd.telescope.backend import PERIOD_DTYPE

    def boom(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_engine, "to_dev", boom)
    monkeypatch.setattr(_engine, "execute", boom)
    be = _Backend()(samprate=0.01, name="B")
    sig = _signal()
    ok = dict(dms=[0.0, 60.0], periods=[0.05, 0.05])              # largest delay 749: T = 15635
    cands = PeriodCandidates(np.zeros(0, dtype=PERIOD_DTYPE), None, 10.0)
    for fn in (be.fold_candidates, be._fold_plan):
        with pytest.raises(ValueError, match="FilterBankSignal"):
            fn(None, **ok)
        with pytest.raises(ValueError, match="search-mode"):
            fn(_signal(fold=True), **ok)
        with pytest.raises(ValueError, match="either candidates or dms and periods"):
            fn(sig)                                                       # neither
        with pytest.raises(ValueError, match="either candidates or dms and periods"):
            fn(sig, candidates=cands, **ok)                               # both
        with pytest.raises(ValueError, match="both dms and periods"):
            fn(sig, dms=[1.0])
        with pytest.raises(ValueError, match="not PeriodCandidates"):
            fn(sig, candidates=[1, 2])
        with pytest.raises(ValueError, match="no candidate"):
            fn(sig, candidates=cands)                                     # K < 1
        with pytest.raises(ValueError, match="no candidate"):
            fn(sig, dms=[], periods=[])
        with pytest.raises(ValueError, match="2 dms for 1 periods"):
            fn(sig, dms=[0.0, 1.0], periods=[0.05])
        for bad in (0.0, -0.05, np.nan, np.inf):
            with pytest.raises(ValueError, match="period is not finite and positive"):
                fn(sig, dms=[0.0, 30.0], periods=[0.05, bad])
        with pytest.raises(ValueError, match="negative or not finite"):
            fn(sig, dms=[0.0, -1.0], periods=[0.05, 0.05])
        with pytest.raises(ValueError, match="shorter than nbin 64 bins -- lower nbin"):
            fn(sig, dms=[0.0], periods=[63.9e-4])                         # 63.9 samples
        with pytest.raises(ValueError, match="nband 7 does not divide the 64 channels"):
            fn(sig, nband=7, **ok)
        with pytest.raises(ValueError, match="nband 0 does not divide"):
            fn(sig, nband=0, **ok)
        with pytest.raises(ValueError, match="nsub 15636 exceeds the 15635 samples"):
            fn(sig, nsub=15636, **ok)
        with pytest.raises(ValueError, match="nsub 0 < 1"):
            fn(sig, nsub=0, **ok)
        for bad in (1, 0, 1025, -4):
            with pytest.raises(ValueError, match="nbin %d outside" % bad):
                fn(sig, nbin=bad, **ok)
        for kw in (dict(nbin=2.5), dict(nsub="x"), dict(nband=None), dict(max_bytes=1.5)):
            with pytest.raises(ValueError, match="integers"):
                fn(sig, **dict(ok, **kw))
        with pytest.raises(ValueError, match="stat_block"):
            fn(sig, stat_block=1, **ok)
        with pytest.raises(ValueError, match=r"one DM \(500352 bytes\) exceed max_bytes 500351"):
            fn(sig, max_bytes=500351, **ok)
        with pytest.raises(ValueError, match="leaves no output sample"):
            fn(_signal(N=700), **ok)
    # at the limits the plan goes through
    p = be._fold_plan(sig, nsub=15635, max_bytes=500352, dms=[60.0], periods=[64e-4])
    assert p["L"] == 1 and p["T"] == 15635 and p["chunks"] == [(0, 1)]


def test_plan_maps_duplicate_dms_to_one_series_and_chunks_cover_them_once():
    be = _Backend()(samprate=0.01, name="B")
    sig = _signal()
    dms = [30.0, 0.0, 60.0, 30.0, 5.0, 0.0, 45.0]
    per = [0.05, 0.05, 0.07, 0.1003, 0.05, 0.0064, 0.05]
    p = be._fold_plan(sig, dms=dms, periods=per, nbin=64, nsub=16, nband=8)
    assert p["K"] == 7 and np.array_equal(p["udms"], [0.0, 5.0, 30.0, 45.0, 60.0])
    assert np.array_equal(p["ju"], [2, 0, 4, 2, 1, 0, 3]) and np.array_equal(p["udms"][p["ju"]], dms)
    assert np.array_equal(p["delays"], be.dedisperse_delays(sig, p["udms"]))
    assert p["max_delay"] == 749 and p["T"] == 16384 - 749 and p["L"] == p["T"] // 16 and p["ld"] == 15636
    assert p["ld"] % 4 == 0 and p["C"] == 64 and p["Cb"] == 8 and p["ref_freq"] == 1593.75
    assert p["chunks"] == [(0, 5)]
    assert p["inc"] == [ref.phase_step(v) for v in p["period_samples"]]
    assert all(isinstance(i, int) for i in p["inc"]) and p["inc"][0] == 36893488147419103
    f = np.asarray(sig.dat_freq.value if hasattr(sig.dat_freq, "value") else sig.dat_freq, dtype=np.float64)
    w = (f ** -2.0 - 1593.75 ** -2.0).reshape(8, 8).mean(axis=1)
    assert np.allclose(p["band_w"], w, rtol=1e-14, atol=0) and p["band_w"].shape == (8,)
    assert np.all(np.diff(p["band_w"]) < 0) and p["band_w"][-1] > 0     # channels rise in frequency
    # chunking: every unique DM exactly once, whatever max_bytes allows
    per_dm = 8 * 15636 * 4
    for mb, want in ((per_dm, 1), (2 * per_dm, 2), (3 * per_dm + 17, 3), (5 * per_dm, 5), (1 << 30, 5)):
        ch = be._fold_plan(sig, dms=dms, periods=per, max_bytes=mb)["chunks"]
        assert ch[0][0] == 0 and ch[-1][1] == 5 and all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        assert max(hi - lo for lo, hi in ch) == want and all(hi > lo for lo, hi in ch)


def test_plan_takes_the_strongest_candidates():
    from psrsigsim_amd.telescope import PeriodCandidates
    from psrsigsim_amd.telescope.backend import PERIOD_DTYPE
    be = _Backend()(samprate=0.01, name="B")
    arr = np.zeros(4, dtype=PERIOD_DTYPE)
    arr["snr"] = [50.0, 40.0, 30.0, 20.0]
    arr["dm"] = [30.0, 25.0, 30.0, 0.0]
    arr["period"] = [0.05, 0.025, 0.1, 0.05]
    c = PeriodCandidates(arr, None, 10.0)
    p = be._fold_plan(_signal(), candidates=c, max_candidates=3)
    assert p["K"] == 3 and np.array_equal(p["dms"], [30.0, 25.0, 30.0])
    assert np.array_equal(p["periods"], [0.05, 0.025, 0.1]) and np.array_equal(p["ju"], [1, 0, 1])
    assert be._fold_plan(_signal(), candidates=c)["K"] == 4
    with pytest.raises(ValueError, match="max_candidates 0 < 1"):
        be._fold_plan(_signal(), candidates=c, max_candidates=0)


# ---------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_hashed():
    from psrsigsim_amd import build
    with open(os.path.join(ROOT, "include", "pss_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+pss_fold_series\s*\(", header)
    assert "pss_fold_series" in _lib.EXPORTS and len(_lib.EXPORTS["pss_fold_series"][1]) == 14
    assert hasattr(_lib.load(), "pss_fold_series")
    assert "pss_foldseries.hip" in build.UNITS
    assert any(os.path.basename(d) == "pss_foldseries.hip" for d in build.DEPS)      # source_hash() covers it


def test_entry_point_validates_arguments():
    """Every PSS_EINVAL of pss_fold_series with NULL or host pointers: the
    checks precede any launch (no GPU touched)."""
    p = host_pointer()
    good = dict(x=p, nser=2, T=16, ld=16, src=p, inc=p, phi0=None, nrows=3, nsub=2, Ls=8, nbin=4, out=p, hits=None)
    check_rejections(_lib.load().pss_fold_series, good,
                   ((dict(x=None), "x is NULL"), (dict(src=None), "src is NULL"), (dict(inc=None), "inc is NULL"),
                    (dict(out=None), "out is NULL"), (dict(nser=0), "nser 0 < 1"), (dict(nrows=0), "nrows 0 < 1"),
                    (dict(nrows=-2), "nrows -2 < 1"), (dict(nsub=0), "nsub 0 < 1"), (dict(Ls=0), "L 0 < 1"),
                    (dict(Ls=9), "nsub 2 x L 9 > T 16"), (dict(nsub=3, Ls=6), "nsub 3 x L 6 > T 16"),
                    (dict(Ls=1 << 62, nsub=4), "x L 4611686018427387904 > T 16"),
                    (dict(ld=15), "ld 15 < T 16"), (dict(nbin=1), "nbin 1 outside [2, 1024]"),
                    (dict(nbin=1025), "nbin 1025 outside [2, 1024]"), (dict(nbin=0), "nbin 0 outside"),
                    (dict(nrows=1 << 30, nsub=2), "exceed 2^31 - 1 workgroups")))


# ---------------------------------------------------------------------------
# refine
# ---------------------------------------------------------------------------
NBAND, NSUB, NBIN, LSUB, PS, FS = 4, 8, 32, 1000, 500.0, 1e4
BAND_W = np.array([3.0, 2.0, 1.0, 0.0]) * 1e-7


def _folded(cube, hits=None, mean=0.0, var=0.25, dm=30.0):
    from psrsigsim_amd.telescope import FoldedCandidates
    cube = np.asarray(cube, dtype=np.float32)
    K = cube.shape[0]
    nsub = cube.shape[2]
    hits = np.full((K, nsub, NBIN), 10, dtype=np.int32) if hits is None else np.asarray(hits, dtype=np.int32)
    return FoldedCandidates(cube, hits, np.full((K, NBAND), mean), np.full((K, NBAND), var), [dm] * K,
                            [PS / FS] * K, [PS] * K, [ref.phase_step(PS)] * K, BAND_W, FS / 1e6, 1593.75, LSUB,
                            nsub * LSUB + 3, 749)


def _pulse(drift, dm_shift, b0=11):
    step = PS / (ref.DM_K * BAND_W.max() * FS * NBIN)
    q = ref.dm_bins(dm_shift, step, BAND_W, FS, PS, NBIN)
    cube = np.zeros((NBAND, NSUB, NBIN))
    for g in range(NBAND):
        for s in range(NSUB):
            cube[g, s, (b0 + ref.drift_shift(drift, s, NSUB) + q[g]) % NBIN] = 1.0
    return cube, step, q


def _check_against_ref(fc, got, k=0, **kw):
    want = ref.refine(fc.cube[k], fc.hits[k], fc.mean[k], fc.var[k], PS, fc.dms[k], BAND_W, FS, LSUB, **kw)
    for name in ("drift", "dm_shift", "peak_bin"):
        assert got[k][name] == want[name], name
    for name in ("chi2", "chi2_opt", "period_opt", "dm_opt"):
        assert np.isclose(got[k][name], want[name], rtol=1e-12, atol=0), name
    assert np.allclose(got[k]["profile"], want["profile"], rtol=1e-12, atol=0)
    return want


def test_refine_recovers_a_drift_and_a_dm_offset():
    cube, step, q = _pulse(5, -3)
    assert q == [-3, -2, -1, 0]
    assert [ref.drift_shift(5, s, NSUB) for s in range(NSUB)] == [0, 1, 2, 2, 3, 3, 4, 5]
    assert [ref.drift_shift(-5, s, NSUB) for s in range(NSUB)] == [0, -1, -2, -2, -3, -3, -4, -5]
    fc = _folded([cube, _pulse(-7, 4, b0=30)[0]])
    assert len(fc) == 2 and "2 candidates x 4 bands x 8 sub-integrations of 1000 samples x 32 bins" in repr(fc)
    assert fc.profile().shape == (2, NBIN) and fc.profile().sum() == 2 * NBAND * NSUB
    with np.errstate(all="raise"):
        got = fc.refine()
    assert got.shape == (2,) and got["profile"].shape == (2, NBIN)
    assert got[0]["drift"] == 5 and got[0]["dm_shift"] == -3 and got[0]["peak_bin"] == 11
    assert got[1]["drift"] == -7 and got[1]["dm_shift"] == 4 and got[1]["peak_bin"] == 30
    assert got[0]["chi2_opt"] > got[0]["chi2"] and got[1]["chi2_opt"] > got[1]["chi2"]
    assert got[0]["profile"][11] == NBAND * NSUB and got[0]["profile"].sum() == NBAND * NSUB
    # all 32 unit pulses in one bin of 80 hits, M = 0, V = 1
    assert np.isclose(got[0]["chi2_opt"], 32.0 ** 2 / 80.0 / 31.0, rtol=1e-14)
    assert got[0]["period"] == PS / FS and got[0]["dm"] == 30.0
    assert got[0]["period_opt"] == 1.0 / (1.0 / PS - 5 / (float(NBIN) * NSUB * LSUB)) / FS
    assert got[0]["period_opt"] > got[0]["period"]            # arriving later and later: folded too short
    assert got[1]["period_opt"] == 1.0 / (1.0 / PS + 7 / (float(NBIN) * NSUB * LSUB)) / FS
    assert got[0]["dm_opt"] == 30.0 - 3 * step and got[1]["dm_opt"] == 30.0 + 4 * step
    _check_against_ref(fc, got, 0)
    _check_against_ref(fc, got, 1)
    # a narrower search cannot reach the drift; an explicit dm_step rescales the shifts
    near = fc.refine(ndrift=2, ndm=1, dm_step=2 * step)
    assert abs(near[0]["drift"]) <= 2 and abs(near[0]["dm_shift"]) <= 1
    _check_against_ref(fc, near, 0, ndrift=2, ndm=1, dm_step=2 * step)
    with pytest.raises(ValueError, match="negative"):
        fc.refine(ndrift=-1)


def test_refine_leaves_an_aligned_pulse_alone():
    cube, _, _ = _pulse(0, 0, b0=3)
    fc = _folded([cube])
    got = fc.refine()
    assert got[0]["drift"] == 0 and got[0]["dm_shift"] == 0 and got[0]["peak_bin"] == 3
    assert got[0]["chi2_opt"] == got[0]["chi2"] > 0
    assert got[0]["period_opt"] == PS / FS and got[0]["dm_opt"] == 30.0
    _check_against_ref(fc, got)


def test_refine_of_a_constant_cube_is_flat():
    # every bin holds mean x hits: chi2 0 at every trial, so every trial ties and (0, 0) wins
    fc = _folded(np.full((1, NBAND, NSUB, NBIN), 2.5 * 10), mean=2.5)
    got = fc.refine()
    assert got[0]["chi2"] == 0.0 and got[0]["chi2_opt"] == 0.0
    assert got[0]["drift"] == 0 and got[0]["dm_shift"] == 0
    _check_against_ref(fc, got)
    # a variance that is not positive gives chi2 0, not a division by zero
    with np.errstate(all="raise"):
        z = _folded(_pulse(2, 1)[0][None], var=0.0).refine()
    assert z[0]["chi2"] == 0.0 and z[0]["chi2_opt"] == 0.0 and z[0]["drift"] == 0 and z[0]["dm_shift"] == 0


def test_refine_ties_go_to_the_smaller_shift_then_the_negative_one():
    from psrsigsim_amd.telescope.backend import _fold_best
    for pick in (_fold_best, lambda c, n: ref.best(dict(zip(range(-n, n + 1), c)), n)):
        assert pick([1.0, 1.0, 1.0, 1.0, 1.0], 2) == 0
        assert pick([3.0, 1.0, 2.0, 1.0, 3.0], 2) == -2            # |i| equal: the smaller i
        assert pick([3.0, 1.0, 2.0, 3.0, 1.0], 2) == 1             # the smaller |i|
        assert pick([1.0, 3.0, 2.0, 3.0, 3.0], 2) == -1
        assert pick([0.0, 0.0, 0.0, 0.0, 5.0], 2) == 2
    # one sub-integration, flat hits: r_0(i) = (i + 1) // 2 only rotates the profile, every drift ties
    cube = np.zeros((1, NBAND, 1, NBIN))
    cube[0, :, 0, 9] = 4.0
    fc = _folded(cube)
    got = fc.refine(ndm=0)
    assert got[0]["drift"] == 0 and got[0]["peak_bin"] == 9
    _check_against_ref(fc, got, ndm=0)


def test_refine_skips_bins_without_hits():
    cube, _, _ = _pulse(3, 2, b0=20)
    hits = np.full((1, NSUB, NBIN), 10, dtype=np.int32)
    hits[0, :, 0:6] = 0                                              # bins no sample fell into
    hits[0, 2, :] = 0
    fc = _folded([cube], hits=hits, mean=0.01)
    with np.errstate(all="raise"):
        got = fc.refine()
    assert np.isfinite(got[0]["chi2"]) and np.isfinite(got[0]["chi2_opt"])
    assert got[0]["drift"] == 3 and got[0]["dm_shift"] == 2 and got[0]["peak_bin"] == 20
    _check_against_ref(fc, got)
    # nothing but empty bins: chi2 0
    none = _folded([cube], hits=np.zeros((1, NSUB, NBIN), dtype=np.int32)).refine()
    assert none[0]["chi2"] == 0.0 and none[0]["chi2_opt"] == 0.0
