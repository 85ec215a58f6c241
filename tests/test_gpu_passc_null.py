"""The fast pass C on 1024-point columns that nulls the always-nulled samples
itself (PairCols::passC_fast32<true>, plan token ``C:null``) and the fix-up
over the f-dependent words that follows it (k_null_fix_list<true>), against
the generic kernels (PSS_FLAG_NO_FAST), bit for bit.

1024-point columns exist only from 2^22 samples (1024 x 4096) on, so the
shapes are a few channels of a shard with an odd start (poff = 1: the first
pair holds only its second channel, the last only its first), as in
tests/test_gpu_passc_cols16.py, whose cases also cover the no-null
instantiation unchanged.

Pass C takes, per 16-sample row segment, a 16-bit window of the mask table's
always bits at table position p0 = (n1 N2 + n20 - i_c) mod N, i_c the integer
part of the channel's mask shift; the fix-up decides the positions whose
answer depends on the fractional part f_c.  Every case therefore computes
(i_c, f_c) on the host from the mask ramp words BEFORE the run and asserts the
properties it is there for (``_edges``): shifts off the 4-, 16- and 32-sample
grids (windows cut by a nibble, straddling two table words), a segment whose
window wraps past the end of the table, and fractional shifts that differ
between the channels (so the f-dependent path decides differently per
channel and the bitwise comparison covers it).  The run's own ramp words are
then checked to be those words."""
import numpy as np
import pytest

from tests.kernel_harness import same_bits

pytestmark = pytest.mark.gpu

PERIOD, DT = 0.005, 20.48e-6


def _signal(fc, bw, nchan, shard, log2n, dm):
    """make_pulses + disperse, still pending (no device work yet)."""
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar, GaussProfile
    from psrsigsim_amd.ism import ISM
    pss.seed(23)
    sig = FilterBankSignal(fc, bw, Nsubband=nchan, fold=False, shard=shard)
    psr = Pulsar(PERIOD, 1.0, profiles=GaussProfile(0.5, 0.05, 1))
    psr.make_pulses(sig, tobs=(1 << log2n) * DT)
    ISM().disperse(sig, dm)
    return sig, psr


def _host_words(fc, bw, nchan, shard, log2n, dm):
    """The mask ramp words the run will get (Pulsar.null: the total delay in
    samples; _engine.plan_pipeline: ramp_words of the shard's channels)."""
    from psrsigsim_amd import _engine
    from psrsigsim_amd._units import to_value
    sig, _ = _signal(fc, bw, nchan, shard, log2n, dm)
    samples = np.asarray(to_value(sig.delay, "ms"), dtype=np.float64) / sig._dt_ms()
    return _engine.ramp_words(samples[np.arange(shard[0], shard[1])], 1 << log2n), sig.nsub


def _split(words, log2n):
    """(i_c, f_c 2^24) of mask_split (csrc/pss_stages.hpp), in integers."""
    w = [int(x) for x in words]
    return [x >> (64 - log2n) for x in w], [((x << log2n) & ((1 << 64) - 1)) >> 40 for x in w]


def _edges(words, log2n):
    """The window properties a case must have, from its ramp words."""
    N = 1 << log2n
    ish, fr = _split(words, log2n)
    assert any(i % 4 for i in ish), ish                  # a window cut inside a nibble of the table
    assert any(i % 16 for i in ish), ish
    assert any(i % 32 for i in ish), ish
    # a window in two table words: sh = (n20 - i) mod 32 > 16 for n20 = 0 or 16
    assert any(((n20 - i) % 32) > 16 for i in ish for n20 in (0, 16)), ish
    # a row segment (start n1 N2 + n20: any multiple of 16) whose window
    # wraps past the end of the table: p0 > N - 16
    wraps = [((i - i % 16) - i) % N for i in ish if i % 16]
    assert wraps and all(p0 > N - 16 for p0 in wraps), (ish, wraps)
    # the fix-up still matters: the channels' fractional shifts differ
    assert len(set(fr)) == len(fr), fr
    return ish


def _run(cfg, null_frac, spy):
    from psrsigsim_amd.telescope import telescope as T
    sig, psr = _signal(*cfg)
    if null_frac is not None:
        psr.null(sig, null_frac)
    spy.clear()
    T.Arecibo().observe(sig, psr, system="Lband_PUPPI", noise=True)
    return sig.data.cpu().numpy()


@pytest.fixture
def ramp_spy(monkeypatch):
    """The mask ramp words of every planned run, by row count."""
    from psrsigsim_amd import _engine
    seen = {}
    real = _engine.plan_pipeline

    def plan(sig, pend, rows, chan0):
        P = real(sig, pend, rows, chan0)
        if "mask_ramp" in P["arrays"]:
            seen[rows] = np.array(P["arrays"]["mask_ramp"], dtype=np.uint64)
        return P
    monkeypatch.setattr(_engine, "plan_pipeline", plan)
    return seen


C3 = (1400, 400, 6, (1, 4))          # C3's band and pulsar; channels 1..3 of 6


@pytest.mark.parametrize("cfg,null_frac,split", [
    (C3 + (22, 100), 0.1, "1024x4096"),                  # C3: null(0.1), DM 100
    (C3 + (22, 100), 0.9, "1024x4096"),                  # nearly full lists, most blocks all hits
    (C3 + (22, 100), 2e-4, "1024x4096"),                 # 3 nulled pulses: most column blocks list nothing
    (C3 + (23, 100), 0.1, "1024x8192"),                  # the second dispatch site
    # five channels of another band and DM: shifts 21, 7, 23, 0 and 26 mod 32
    ((820, 200, 8, (3, 8), 22, 37.3), 0.3, "1024x4096"),
], ids=["c3_null0.1", "null0.9", "null3pulses", "1024x8192", "shifts_mod32"])
def test_passc_null_bitwise_equals_generic(cfg, null_frac, split, hip_lib, ramp_spy):
    from psrsigsim_amd import _lib
    from tests import replay
    L = _lib.lib()
    log2n, rows = cfg[4], cfg[3][1] - cfg[3][0]
    n2 = int(split.split("x")[1])
    words, nsub = _host_words(*cfg)
    ish = _edges(words, log2n)
    if null_frac < 1e-3:
        # a nulled pulse (and only it holds always-nulled samples) spans
        # PERIOD / DT samples: the 16-column blocks it can touch, against
        # the N2 / 16 of a channel -- most blocks have an empty list
        npulse = int(np.round(nsub * null_frac))
        assert 0 < npulse * (int(np.ceil(PERIOD / DT / 16)) + 2) < n2 // 16 // 2, npulse
    if cfg[:4] != C3:
        assert any(i % 32 == 0 for i in ish) and len({i % 4 for i in ish}) == 4, ish
    _lib.plan_collect()
    fast = _run(cfg, null_frac, ramp_spy)
    replay.assert_plan(_lib.plan_collect(), rows, 1 << log2n,
                       ("fourstep", split, "C:fast", "C:cols16x2", "C:null", "N:table", "N:fix_list"),
                       absent=("A:generic", "C:generic"))
    assert fast.shape == (rows, 1 << log2n)
    np.testing.assert_array_equal(ramp_spy[rows], words)     # the run's words are the ones checked above
    old = L.pss_set_flags(_lib.FLAG_NO_FAST)
    try:
        _lib.plan_collect()
        generic = _run(cfg, null_frac, ramp_spy)
    finally:
        L.pss_set_flags(old)
    replay.assert_plan(_lib.plan_collect(), rows, 1 << log2n, ("fourstep", split, "C:generic"),
                       absent=("C:fast", "C:cols16x2", "C:null"))
    diff = np.flatnonzero((fast.view(np.uint32) != generic.view(np.uint32)).any(axis=0))
    assert same_bits(fast, generic), ("%d columns differ, first at sample %d (column block %d)"
                                      % (diff.size, diff[0], (diff[0] % n2) // 16))


def test_no_null_plan_has_no_passc_null(hip_lib, ramp_spy):
    """Without a null there is no table: the parent's kernel (the NULLC =
    false instantiation; its bits: tests/test_gpu_passc_cols16.py)."""
    from psrsigsim_amd import _lib
    from tests import replay
    _lib.lib()
    _lib.plan_collect()
    out = _run((1400, 400, 2, None, 22, 100), None, ramp_spy)
    assert out.shape == (2, 1 << 22) and not ramp_spy
    replay.assert_plan(_lib.plan_collect(), 2, 1 << 22, ("fourstep", "1024x4096", "C:fast", "C:cols16x2"),
                       absent=("C:null", "N:table", "N:fix_list", "C:generic"))
