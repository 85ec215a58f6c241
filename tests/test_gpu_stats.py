"""Stochastic stages on the GPU (Philox draws): distributions against the
reference's (chi2 via scipy), per-channel moments against the CPU oracle, and
shard invariance (a sharded run reproduces the unsharded rows bit for bit)."""
import numpy as np
import pytest
import torch
from scipy import stats

from oracle import pss_cpu as O

pytestmark = pytest.mark.gpu


def _fill(df, rows=2, n=1 << 20, purpose=5, call=7):
    from psrsigsim_amd import _lib, _engine
    out = torch.empty((rows, n), dtype=torch.float32, device="cuda")
    rc = _lib.lib().pss_chi2_fill(_engine.ptr(out), rows, 0, n, float(df), 1234, call, purpose,
                                  _engine.stream_ptr())
    _lib.check(rc)
    return out.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("df", [1.0, 0.5, 3.7, 100.0, 11190.0])
def test_chi2_draws_distribution(df, hip_lib):
    """Mean within 0.5 % and variance within 1 % of chi2(df) per row (or 4
    standard errors, whichever is larger: chi2's fourth central moment is
    12 df (df + 4), so at df = 0.5 the sample variance of 2^20 draws has a
    0.5 % standard error -- 2^24 draws per row are used for df < 2), plus a
    KS test (p > 0.01)."""
    n = 1 << (24 if df < 2 else 20)
    x = _fill(df, n=n)
    se_m = np.sqrt(2.0 / (df * n))                                   # relative SE of the mean
    se_v = np.sqrt((12.0 * df * (df + 4) - 4.0 * df * df) / n) / (2.0 * df)   # ... of the variance
    for row in x:
        m, v = row.mean(), row.var()
        assert abs(m / df - 1) < max(5e-3, 4 * se_m), (df, m)
        assert abs(v / (2 * df) - 1) < max(1e-2, 4 * se_v), (df, v)
        p = stats.kstest(row[:200000], stats.chi2(df).cdf).pvalue
        assert p > 0.01, (df, p)


def test_chi2_streams_independent(hip_lib):
    a = _fill(1.0, call=1)[0]
    b = _fill(1.0, call=2)[0]
    assert abs(np.corrcoef(a[:100000], b[:100000])[0, 1]) < 0.02


def _c3_small(nchan, shard, log2n=16, noise=True, seed=5):
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar, GaussProfile
    from psrsigsim_amd.ism import ISM
    from psrsigsim_amd.telescope import telescope as T
    pss.seed(seed)
    sig = FilterBankSignal(1400, 400, Nsubband=nchan, fold=False, shard=shard)
    psr = Pulsar(0.005, 1.0, profiles=GaussProfile(0.5, 0.05, 1))
    ism = ISM()
    ism.scatter_broaden(sig, 1e-4, 1400, convolve=True, pulsar=psr)
    psr.make_pulses(sig, tobs=(1 << log2n) * 20.48e-6)
    ism.disperse(sig, 100)
    psr.null(sig, 0.1)
    T.Arecibo().observe(sig, psr, system="Lband_PUPPI", noise=noise)
    return sig.data.cpu().numpy()


@pytest.mark.parametrize("log2n", [13, 16])
def test_shard_invariance_bitwise(log2n, hip_lib):
    """Even shard boundaries (the four-step path pairs global channels
    (2q, 2q+1) in one complex row, so a pair must not straddle a shard)."""
    full = _c3_small(8, None, log2n)
    a = _c3_small(8, (0, 2), log2n)
    b = _c3_small(8, (2, 8), log2n)
    np.testing.assert_array_equal(np.vstack([a, b]), full)


@pytest.mark.parametrize("nchan,log2n,null,dm", [(3, 16, True, 100), (4, 17, True, 100), (5, 14, True, 100),
                                                (2, 16, False, 100), (3, 22, True, 100),
                                                # C5's per-GPU geometry: 2^24 (2048 x 8192 split), DM 500
                                                (2, 24, True, 500),
                                                # 3 125 000 = 2^3 5^8 (radix-5 four-step 1250 x 2500; fast
                                                # passes A and C; no delayed null off 2^m lengths)
                                                (3, None, False, 100)])
def test_fast_path_bitwise_equals_generic(nchan, log2n, null, dm, hip_lib):
    """The fast-path kernels (Philox df=1, no injection: the north-star
    configuration) against the generic kernels, bit for bit."""
    from psrsigsim_amd import _lib

    def run():
        import psrsigsim_amd as pss
        from psrsigsim_amd.signal import FilterBankSignal
        from psrsigsim_amd.pulsar import Pulsar, GaussProfile
        from psrsigsim_amd.ism import ISM
        from psrsigsim_amd.telescope import telescope as T
        pss.seed(11)
        sig = FilterBankSignal(1400, 400, Nsubband=nchan, fold=False)
        psr = Pulsar(0.005, 1.0, profiles=GaussProfile(0.5, 0.05, 1))
        psr.make_pulses(sig, tobs=(1 << log2n) * 20.48e-6 if log2n else 64.0)   # 64 s: 3 125 000 samples
        ISM().disperse(sig, dm)
        if null:
            psr.null(sig, 0.2)
        T.Arecibo().observe(sig, psr, system="Lband_PUPPI", noise=True)
        return sig.data.cpu().numpy()

    L = _lib.lib()
    fast = run()
    if log2n is None:
        assert fast.shape[1] == 3125000
    if (log2n or 22) >= 22:
        # run to run: a kernel reading LDS it did not write (stale from an
        # earlier workgroup) shows up here even when both paths share it
        np.testing.assert_array_equal(run(), fast)
    old = L.pss_set_flags(_lib.FLAG_NO_FAST)
    try:
        generic = run()
    finally:
        L.pss_set_flags(old)
    np.testing.assert_array_equal(fast, generic)


F0_B1855 = 186.4940812499314404


# the split each (tobs, bins) geometry below must take (asserted in the launch plan)
FOLD_SPLITS = {(1800.0, 1024): "30x1024", (600.0, 1024): "10x1024", (720.0, 2048): "6x4096"}


@pytest.mark.parametrize("nchan,shard,tobs,samprate_bins", [
    (4, None, 1800.0, 1024),          # C4's geometry: 30 x 1024 (register columns, 30-point DFT)
    (5, (1, 4), 1800.0, 1024),        # odd shard start: pair (0, 1) misses channel 0
    (3, None, 600.0, 1024),           # 10 subints: 10 x 1024
    (2, None, 720.0, 2048),           # 12 subints of 2048 bins: 24576 samples = 6 x 4096
])
def test_fold_fast_bitwise_equals_generic(nchan, shard, tobs, samprate_bins, hip_lib):
    """Fold mode on the mixed-radix split: the fold fast kernels
    (k_pairA_fold / k_pairC_fold: chi2(Nfold) pair draws split over the
    lanes of a column pair, one DPP swap) against the generic kernels
    (source4 / epilogue4 draws through LDS), bit for bit; the generic path is
    itself checked against the oracle with injected draws
    (test_gpu_parity.py::test_c4_fold_mixed_radix_vs_oracle).  The launch plan
    of each run must show the split named above and its kernels."""
    from psrsigsim_amd import _lib
    from tests import replay
    rows = shard[1] - shard[0] if shard else nchan
    nsamp = int(round(tobs / 60.0)) * samprate_bins
    split = FOLD_SPLITS[(tobs, samprate_bins)]

    def run():
        import psrsigsim_amd as pss
        from psrsigsim_amd.signal import FilterBankSignal
        from psrsigsim_amd.pulsar import Pulsar, GaussProfile
        from psrsigsim_amd.ism import ISM
        from psrsigsim_amd.telescope import telescope as T
        pss.seed(29)
        sig = FilterBankSignal(1400, 400, Nsubband=nchan, sample_rate=F0_B1855 * samprate_bins * 1e-6,
                               sublen=60.0, fold=True, shard=shard)
        psr = Pulsar(1.0 / F0_B1855, 0.005, profiles=GaussProfile(0.5, 0.05, 1))
        psr.make_pulses(sig, tobs=tobs)
        ISM().disperse(sig, 13.299393)
        T.Arecibo().observe(sig, psr, system="Lband_PUPPI", noise=True)
        return sig.data.cpu().numpy()

    L = _lib.lib()
    _lib.plan_collect()
    fast = run()
    replay.assert_plan(_lib.plan_collect(), rows, nsamp, ("smooth", split, "A:fold", "C:fold"),
                       absent=("A:generic", "C:generic"))
    assert np.isfinite(fast).all()
    old = L.pss_set_flags(_lib.FLAG_NO_FAST)
    try:
        _lib.plan_collect()
        generic = run()
    finally:
        L.pss_set_flags(old)
    replay.assert_plan(_lib.plan_collect(), rows, nsamp, ("smooth", split, "A:generic", "C:generic"),
                       absent=("A:fold", "C:fold"))
    np.testing.assert_array_equal(fast, generic)


def test_shard_invariance_odd_boundary_close(hip_lib):
    """Odd boundary: bit-for-bit only up to the pair partner's rounding."""
    full = _c3_small(8, None, 16)
    a = _c3_small(8, (0, 3), 16)
    b = _c3_small(8, (3, 8), 16)
    got = np.vstack([a, b])
    err = np.max(np.abs(got - full), axis=1) / np.max(np.abs(full), axis=1)
    assert np.all(err < 1e-5), err


def test_pulse_and_noise_moments_vs_oracle(hip_lib):
    """Per-channel mean and variance of the final C3-style signal (Philox)
    against the oracle (legacy RandomState) within 0.5 % + sampling error."""
    log2n = 20
    g = _c3_small(2, None, log2n)
    sig = O.Signal(1400, 400, nchan=2, fold=False)
    psr = O.Pulsar(0.005, 1.0, profiles=O.GaussPortrait(0.5, 0.05, 1))
    d = O.LegacyDraws(3)
    O.scatter_broaden(sig, 1e-4, 1400, convolve=True, pulsar=psr)
    O.make_pulses(sig, psr, (1 << log2n) * 20.48e-6, d)
    O.disperse(sig, 100)
    O.null(sig, psr, 0.1, d)
    O.observe(sig, psr, O.Arecibo(), "Lband_PUPPI", d, noise=True)
    for c in range(2):
        x, y = g[c].astype(np.float64), sig.data[c]
        n = x.size
        for stat, se in ((np.mean, lambda a: a.std() / np.sqrt(n)),
                         (np.var, lambda a: np.sqrt(np.mean((a - a.mean()) ** 4) / n))):
            sx, sy = stat(x), stat(y)
            tol = max(5e-3 * abs(sy), 5 * np.hypot(se(x), se(y)))
            assert abs(sx - sy) <= tol, (c, stat.__name__, sx, sy, tol)


def test_search_pulse_draws_are_chi2_1(hip_lib):
    """make_pulses alone (no delay): data / PCHIP(phase) ~ chi2(1), on the
    on-pulse samples of eight seeds pooled (8 x 61 486: one KS test, p >
    0.01, and the mean).  The device stream follows the NumPy model of
    tests/philox_ref.py draw for draw (tests/test_gpu_draw_streams.py), and
    the 400-seed study of this very statistic by tools/philox_model.py
    (profiles/r03/philox_quality.txt) shows uniform p-values for
    Philox4x32-7 as for -10."""
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar, GaussProfile
    pooled = []
    for seed in range(11, 19):
        pss.seed(seed)
        sig = FilterBankSignal(1400, 400, Nsubband=2, fold=False)
        psr = Pulsar(0.005, 1.0, profiles=GaussProfile(0.5, 0.1, 1))
        psr.make_pulses(sig, tobs=(1 << 18) * 20.48e-6)
        x = sig.data.cpu().numpy().astype(np.float64)
        spp = (sig._samprate_MHz() * 0.005) * 1e6
        ph = (np.arange(x.shape[1]) / spp) % 1
        prof = psr.Profiles.calc_profiles(ph)
        sel = prof[0] > 0.5
        r = x[0, sel] / prof[0, sel]
        pooled.append(r)
    r = np.concatenate(pooled)
    assert stats.kstest(r, stats.chi2(1).cdf).pvalue > 0.01
    assert abs(r.mean() - 1) < 5e-3


def test_radiometer_noise_distribution(hip_lib):
    """observe(noise=True): (after - before) / norm ~ chi2(df), df = Nfold =
    10 (fold mode): 20 s of 2 channels, 195 200 draws, so the 0.5 % bound on
    the mean is ~5 standard errors (sqrt(2 df / n) / df = 1e-3)."""
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar, GaussProfile
    from psrsigsim_amd.telescope import telescope as T
    from psrsigsim_amd.telescope.receiver import Receiver
    pss.seed(12)
    sig = FilterBankSignal(1400, 400, Nsubband=2, sublen=0.05)
    psr = Pulsar(0.005, 1.0, profiles=GaussProfile(0.5, 0.05, 1))
    psr.make_pulses(sig, tobs=20.0)
    before = sig.data.cpu().numpy().astype(np.float64)
    tel = T.Arecibo()
    tel.observe(sig, psr, system="Lband_PUPPI", noise=True)
    after = sig.data.cpu().numpy().astype(np.float64)
    norm = Receiver.noise_norm(sig, psr, tel.Tsys, tel.gain)
    df = float(sig.Nfold)
    z = ((after - before) / norm).ravel()
    assert abs(z.mean() / df - 1) < 5e-3
    assert stats.kstest(z, stats.chi2(df).cdf).pvalue > 0.01


def _bs_small(nchan, shard, nsamp=10006, seed=9):
    """A search-mode run on a Bluestein length (no null: pair mode, two
    channels per complex row, source / epilogue fused into the column passes)."""
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar, GaussProfile
    from psrsigsim_amd.ism import ISM
    from psrsigsim_amd.telescope import telescope as T
    pss.seed(seed)
    sig = FilterBankSignal(1400, 400, Nsubband=nchan, fold=False, shard=shard)
    psr = Pulsar(0.005, 1.0, profiles=GaussProfile(0.5, 0.05, 1))
    psr.make_pulses(sig, tobs=(nsamp + 0.5) * 20.48e-6)
    ISM().disperse(sig, 100)
    T.Arecibo().observe(sig, psr, system="Lband_PUPPI", noise=True)
    return sig.data.cpu().numpy()


@pytest.mark.parametrize("shards", [((0, 2), (2, 6), (6, 7)), ((0, 3), (3, 7)), ((0, 1), (1, 4), (4, 7))])
def test_bluestein_pair_mode_shards(shards, hip_lib):
    """Bluestein pair mode over shards (pairs of GLOBAL channels (2q, 2q+1);
    a shard starting at an odd channel has a lone first row, one ending at an
    even channel a lone last row): even boundaries bit for bit, odd ones
    within the pair partner's rounding; the whole band against the oracle's
    statistics is covered by test_bluestein_pipeline_vs_oracle."""
    full = _bs_small(7, None)
    parts = [_bs_small(7, s) for s in shards]
    got = np.vstack(parts)
    assert got.shape == full.shape
    for (c0, c1), p in zip(shards, parts):
        if c0 % 2 == 0 and (c1 % 2 == 0 or c1 == 7):
            np.testing.assert_array_equal(p, full[c0:c1])
    err = np.max(np.abs(got - full), axis=1) / np.max(np.abs(full), axis=1)
    assert np.all(err < 1e-5), err
