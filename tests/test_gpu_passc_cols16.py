"""The register-resident fast pass C on 1024-point columns (k_pairC_fast32 on
16-column blocks of 512 threads, two workgroups per CU; plan token
``C:cols16x2``) against the generic kernels (PSS_FLAG_NO_FAST), bit for bit,
at its three dispatch sites: 2^22 = 1024 x 4096, 2^23 = 1024 x 8192 and
2^24 = 1024 x 16384 (no delayed null there: with one, 2^24 takes the
2048 x 8192 split).  1024-point columns exist only from 2^22 samples on, so
the small shapes have few channels, not short rows.

The odd shard start makes poff = 1: the first pair holds only its second
channel and the last pair only its first (hasa / hasb false), and the delayed
null puts k_null_fix_list after the new kernel.  The generic kernels are
themselves checked against the float64 oracle (tests/test_gpu_parity.py,
tests/test_gpu_fastpath_oracle.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _run(nchan, shard, log2n, null):
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar, GaussProfile
    from psrsigsim_amd.ism import ISM
    from psrsigsim_amd.telescope import telescope as T
    pss.seed(23)
    sig = FilterBankSignal(1400, 400, Nsubband=nchan, fold=False, shard=shard)
    psr = Pulsar(0.005, 1.0, profiles=GaussProfile(0.5, 0.05, 1))
    psr.make_pulses(sig, tobs=(1 << log2n) * 20.48e-6)
    ISM().disperse(sig, 100)
    if null:
        psr.null(sig, 0.1)
    T.Arecibo().observe(sig, psr, system="Lband_PUPPI", noise=True)
    return sig.data.cpu().numpy()


@pytest.mark.parametrize("nchan,shard,log2n,null,split", [
    (6, (1, 4), 22, True, "1024x4096"),       # poff = 1: both edge pairs miss a channel; null fix-up after
    (2, None, 22, False, "1024x4096"),
    (2, None, 23, True, "1024x8192"),
    (2, None, 24, False, "1024x16384"),       # n20 up to 16368
])
def test_passc_cols16_bitwise_equals_generic(nchan, shard, log2n, null, split, hip_lib):
    from psrsigsim_amd import _lib
    from tests import replay
    L = _lib.lib()
    rows = shard[1] - shard[0] if shard else nchan
    _lib.plan_collect()
    fast = _run(nchan, shard, log2n, null)
    want = ("fourstep", split, "C:fast", "C:cols16x2") + (("N:table", "N:fix_list") if null else ())
    replay.assert_plan(_lib.plan_collect(), rows, 1 << log2n, want, absent=("A:generic", "C:generic"))
    assert fast.shape == (rows, 1 << log2n)
    # run to run: a kernel reading LDS it did not write would differ here
    # even where both paths shared the fault
    np.testing.assert_array_equal(_run(nchan, shard, log2n, null), fast)
    old = L.pss_set_flags(_lib.FLAG_NO_FAST)
    try:
        _lib.plan_collect()
        generic = _run(nchan, shard, log2n, null)
    finally:
        L.pss_set_flags(old)
    replay.assert_plan(_lib.plan_collect(), rows, 1 << log2n, ("fourstep", split, "C:generic"),
                       absent=("C:fast", "C:cols16x2"))
    np.testing.assert_array_equal(fast, generic)
