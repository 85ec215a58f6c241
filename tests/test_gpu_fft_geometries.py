"""Every FFT plan geometry of tests/fft_geometries.py on the device.

(a) Delay rows against the float64 oracle at every delay-only geometry (the
    lengths the sweep of tests/test_gpu_parity.py does not already run), with
    the geometry's kernels asserted in the launch plan.
(b) The search-mode fast passes against the generic kernels, bit for bit, at
    the power-of-two splits and the register-column mixed-radix splits where
    they had never run.
(c) The fold-mode fast passes against the generic kernels, bit for bit, at
    every column length on 8192-point rows (and 30 x 2048).
(d) The generic passes of those geometries against the oracle with injected
    draws -- with (b) and (c) this ties the fast kernels to the oracle.

Tolerance of the oracle comparisons: per-row max|d| / max|ref| <= 1e-5 (fp32
device against a float64 reference, BASELINE.json north_star)."""
import numpy as np
import pytest

from tests import fft_geometries as G
from tests import replay

pytestmark = pytest.mark.gpu
TOL = 1e-5
F0_B1855 = 186.4940812499314404
GENERIC = ("A:generic", "C:generic")


# ---------------------------------------------------------------------------
# (a) delay rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [n for n in G.delay_lengths() if n not in G.PARITY_SWEEP])
def test_shift_t_rows_every_geometry(N, hip_lib):
    G.check_shift_rows(N, TOL)


# ---------------------------------------------------------------------------
# (b) search-mode fast passes == generic
# ---------------------------------------------------------------------------
def _search_signal(N, nchan, null, dtype=np.float32, period=0.005):
    """(signal, pulsar) with make_pulses, disperse and (``null``) a delayed
    null pending: nothing has run yet, and observe() is the caller's."""
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar, GaussProfile
    from psrsigsim_amd.ism import ISM
    pss.seed(31)
    sig = FilterBankSignal(1400, 400, Nsubband=nchan, fold=False, dtype=dtype)
    psr = Pulsar(period, 1.0, profiles=GaussProfile(0.5, 0.05, 1))
    psr.make_pulses(sig, tobs=(N + 0.5) * 20.48e-6)
    assert sig.nsamp == N
    ISM().disperse(sig, 100)
    if null:
        psr.null(sig, 0.2)
    return sig, psr


def _search_run(N, nchan, null):
    from psrsigsim_amd.telescope import telescope as T
    sig, psr = _search_signal(N, nchan, null)
    T.Arecibo().observe(sig, psr, system="Lband_PUPPI", noise=True)
    return sig.data.cpu().numpy()


def _fast_vs_generic(run, nrows, N, tokens, fast):
    """run() with the fast kernels (plan: tokens + fast, no generic pass) and
    under PSS_FLAG_NO_FAST (plan: both generic passes): the same bits."""
    from psrsigsim_amd import _lib
    L = _lib.lib()
    _lib.plan_collect()
    a = run()
    replay.assert_plan(_lib.plan_collect(), nrows, N, tokens + fast, absent=GENERIC)
    assert a.shape == (nrows, N) and np.isfinite(a).all()
    old = L.pss_set_flags(_lib.FLAG_NO_FAST)
    try:
        _lib.plan_collect()
        b = run()
    finally:
        L.pss_set_flags(old)
    replay.assert_plan(_lib.plan_collect(), nrows, N, tokens + GENERIC, absent=fast)
    np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("N", [1 << 15, 1 << 18, 1 << 19, 1 << 20, 1 << 21, 1 << 23,
                               98304, 163840, 196608, 327680, 393216, 491520])
def test_search_fast_bitwise_equals_generic(N, hip_lib):
    """k_pairA_fast / k_pairC_fast (Philox chi2(1) draws, noise, no copy)
    against k_pairA / k_pairC: with a delayed null at the 2^m lengths (mask
    table and k_null_fix_list), without one on the register columns N1 = 12
    .. 60 of the mixed-radix split."""
    null = N & (N - 1) == 0
    g = G.of_length(N, 1 if null else 0)
    assert g.search_fast, g
    fast = G.fast_tokens(g, shared_profile=True) + (("N:fix_list",) if null else ())
    _fast_vs_generic(lambda: _search_run(N, 3, null), 3, N, g.tokens + (("N:table",) if null else ()), fast)


def test_search_fast_mask_table_forked_before_pass_a(hip_lib):
    """The delayed null's mask table forked onto the side stream BEFORE pass A
    (more channels than kMaskAfterANchan = 1024 of csrc/pss_fourstep.hpp; the
    3-channel cases above fork after pass A): the fast run waits for the table
    before the fix-up, the generic run before pass C.  The smallest four-step
    length (16 x 1024) at the smallest even channel count above the threshold."""
    N, nchan = 1 << 14, 1026            # kMaskAfterANchan + 2 (not readable from the library)
    g = G.of_length(N, 1)
    assert g.search_fast, g
    fast = G.fast_tokens(g, shared_profile=True) + ("N:fix_list",)
    _fast_vs_generic(lambda: _search_run(N, nchan, True), nchan, N, g.tokens + ("N:table",), fast)


# ---------------------------------------------------------------------------
# (c) fold-mode fast passes == generic
# ---------------------------------------------------------------------------
def _fold_signal(nchan, shard, nsub, bins):
    """(signal, pulsar) of the fold-mode chain with make_pulses and disperse pending."""
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar, GaussProfile
    from psrsigsim_amd.ism import ISM
    pss.seed(37)
    sig = FilterBankSignal(1400, 400, Nsubband=nchan, sample_rate=F0_B1855 * bins * 1e-6, sublen=60.0,
                           fold=True, shard=shard)
    psr = Pulsar(1.0 / F0_B1855, 0.005, profiles=GaussProfile(0.5, 0.05, 1))
    psr.make_pulses(sig, tobs=60.0 * nsub)
    # (the run's length is the data's nsub * bins columns: signal.nsamp, the
    # reference's int(nsub * (P * samprate) * 1e6), truncates to one less at
    # 60 x 8192 and 30 x 2048; the caller checks the shape and the plan line)
    assert sig._ncols == nsub * bins
    ISM().disperse(sig, 13.299393)
    return sig, psr


def _fold_run(nchan, shard, nsub, bins):
    from psrsigsim_amd.telescope import telescope as T
    sig, psr = _fold_signal(nchan, shard, nsub, bins)
    T.Arecibo().observe(sig, psr, system="Lband_PUPPI", noise=True)
    return sig.data.cpu().numpy()


@pytest.mark.parametrize("nchan,shard,nsub,bins", [
    (3, None, 12, 8192), (3, None, 20, 8192), (3, None, 24, 8192),
    (3, None, 40, 8192),          # T = 128 launches from here on
    (3, None, 48, 8192),          # the swizzled 48-point LDS columns; one fold pass-C wave per SIMD
    (5, (1, 4), 48, 8192),        # odd shard start: pair (0, 1) misses channel 0
    (3, None, 60, 8192),
    (3, None, 30, 2048),
])
def test_fold_fast_every_column_length(nchan, shard, nsub, bins, hip_lib):
    """k_pairA_fold / k_pairC_fold (nsub subintegrations of `bins` phase
    bins: nsub-point register columns) against the generic kernels."""
    N = nsub * bins
    g = G.find("smooth", nsub, bins, 0)
    assert g.nsamp == N and g.fold_fast == ("A:fold", "C:fold")
    nrows = shard[1] - shard[0] if shard else nchan
    _fast_vs_generic(lambda: _fold_run(nchan, shard, nsub, bins), nrows, N, g.tokens, g.fold_fast)


# ---------------------------------------------------------------------------
# (d) the generic passes against the oracle (injected draws)
# ---------------------------------------------------------------------------
def _search_case(N, nchan, null):
    """The C3-style chain of test_gpu_parity._big_case at N samples (the
    delayed null only at 2^m: elsewhere it leaves the four-step)."""
    ops = [("scatter_conv", 1e-4, 1400, None), ("make_pulses", (N + 0.5) * 20.48e-6, "pulses"),
           ("disperse", 100, "disperse"), ("fd", [2e-4, -3e-5], "fd")]
    if null:
        ops.append(("null", 0.1, "null"))
    ops.append(("observe", "Arecibo", "Lband_PUPPI", True, "noise"))
    return dict(sig=dict(fcent=1400, bw=400, nchan=nchan, fold=False),
                psr=dict(period=0.005, Smean=1.0, prof=("gauss", 0.5, 0.05, 1)), ops=ops)


def _fold_case(nsub, bins, nchan):
    """test_gpu_parity._c4_case's fold-mode chain at nsub x bins samples."""
    ops = [("make_pulses", 60.0 * nsub, "pulses"), ("disperse", 13.299393, "disperse"),
           ("observe", "Arecibo", "Lband_PUPPI", True, "noise")]
    return dict(sig=dict(fcent=1400, bw=400, nchan=nchan, samprate=F0_B1855 * bins * 1e-6, sublen=60.0, fold=True),
                psr=dict(period=1.0 / F0_B1855, Smean=0.005, prof=("gauss", 0.5, 0.05, 1)), ops=ops)


def _oracle_case(case, seed, nchan, N, g):
    from psrsigsim_amd import _lib
    _lib.plan_collect()
    errs = replay.run_case(None, fused=True, case=case, seed=seed)
    # the fused run of the whole chain is the one that notes the split
    split = g.tokens[1]
    lines = [l for l in _lib.plan_collect() if split in l.split()]
    replay.assert_plan(lines, nchan, N, g.tokens + GENERIC)
    print("oracle %s N=%d: %s" % (G.gid(g), N, errs))
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert errs and not bad, errs


@pytest.mark.parametrize("N", [1 << 19, 1 << 21, 98304, 163840, 327680, 393216, 491520])
def test_search_generic_vs_oracle(N, hip_lib):
    null = N & (N - 1) == 0
    _oracle_case(_search_case(N, 3, null), N % 1000 + 3, 3, N, G.of_length(N, 1 if null else 0))


@pytest.mark.parametrize("nsub", [12, 20, 40, 48, 60])
def test_fold_generic_vs_oracle(nsub, hip_lib):
    N = nsub * 8192
    _oracle_case(_fold_case(nsub, 8192, 3), nsub, 3, N, G.find("smooth", nsub, 8192, 0))
