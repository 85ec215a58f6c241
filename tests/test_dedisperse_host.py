"""Host side of the incoherent dedispersion (no GPU): the integer delay table
against an independent float64 restatement, a sharded signal's columns, every
Python-level rejection (nothing reaches the device) and the C ABI's argument
checks, which precede any launch."""
import numpy as np
import pytest

from psrsigsim_amd import _lib
from tests.kernel_harness import backend as _backend, check_rejections, host_pointer

DMS = np.arange(0, 65, 5)


class _StubBuf(object):
    """Stands in for the device buffer: any use of it is an error."""

    def __getattr__(self, name):
        raise AssertionError("the device buffer was touched (%s)" % name)


def _fb(nchan=64, n=16384, rate=0.01, fold=False, data=True, shard=None):
    from psrsigsim_amd.signal import FilterBankSignal
    sig = FilterBankSignal(1400, 400, Nsubband=nchan, sample_rate=rate, fold=fold, shard=shard)
    if data:
        sig._buf = _StubBuf()
        sig._ncols = n
        sig._nsamp = n
    return sig


def _restated(dms, nchan=64, fcent=1400.0, bw=400.0, rate_mhz=0.01, ref=None):
    """d[j][c] = floor(K dm_j (f_c^-2 - f_ref^-2) fs + 1/2), K = 1 / 2.41e-4
    MHz^2 s cm^3 / pc, f_c the channels' lower edges, one scalar at a time."""
    f = [fcent - bw / 2 + c * (bw / nchan) for c in range(nchan)]
    ref = max(f) if ref is None else ref
    out = np.empty((len(dms), nchan), dtype=np.int64)
    for j, dm in enumerate(dms):
        for c, fc in enumerate(f):
            x = (1.0 / 2.41e-4) * float(dm) * (1.0 / (fc * fc) - 1.0 / (ref * ref)) * (rate_mhz * 1e6)
            out[j, c] = int(np.floor(x + 0.5))
    return out


def test_delay_table_against_restatement():
    from psrsigsim_amd.telescope import Backend
    d = Backend.dedisperse_delays(_fb(data=False), DMS)
    assert d.dtype == np.int32 and d.shape == (13, 64)
    assert np.array_equal(d, _restated(DMS))
    assert np.all(d[0] == 0)                  # DM 0
    assert np.all(d[:, -1] == 0)              # the top channel is the reference (1593.75 MHz)
    assert np.all(np.diff(d.astype(np.int64), axis=0) >= 0)      # non-decreasing in DM
    assert d.max() == 749
    assert d.max() == d[-1, 0]                # DM 60, 1200 MHz
    # an explicit reference above the band: every delay grows by the same per-DM offset
    d2 = Backend.dedisperse_delays(_fb(data=False), DMS, ref_freq=2000.0)
    assert np.array_equal(d2, _restated(DMS, ref=2000.0))
    assert np.all(d2[1:, -1] > 0)


def test_sharded_signal_gives_its_columns():
    from psrsigsim_amd.telescope import Backend
    full = Backend.dedisperse_delays(_fb(data=False), DMS)
    part = Backend.dedisperse_delays(_fb(data=False, shard=(16, 48)), DMS)
    assert part.shape == (13, 32)
    assert np.array_equal(part, full[:, 16:48])      # common reference: the whole band's top channel
    dm, delays, fref, max_delay, C, N = _backend()._dedisperse_plan(_fb(shard=(16, 48)), DMS)
    assert (C, N, fref) == (32, 16384, 1593.75) and max_delay == full[:, 16:48].max()


def test_rejections_never_reach_the_device(monkeypatch):
    from psrsigsim_amd import _engine
    from psrsigsim_amd.signal import BasebandSignal
    from psrsigsim_amd.telescope import Backend

    def boom(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_engine, "to_dev", boom)
    monkeypatch.setattr(_engine, "execute", boom)
    be = _backend()
    for bad in ([-1.0], [0.0, -5.0], [np.nan], [1.0, np.inf]):
        with pytest.raises(ValueError, match="negative or not finite"):
            Backend.dedisperse_delays(_fb(data=False), bad)
        with pytest.raises(ValueError, match="negative or not finite"):
            be.dedisperse(_fb(), bad)
    for empty in ([], np.zeros(0)):
        with pytest.raises(ValueError, match="empty"):
            Backend.dedisperse_delays(_fb(data=False), empty)
        with pytest.raises(ValueError, match="empty"):
            be.dedisperse(_fb(), empty)
    with pytest.raises(ValueError, match="below a channel frequency"):
        Backend.dedisperse_delays(_fb(data=False), DMS, ref_freq=1500.0)
    with pytest.raises(ValueError, match="below a channel frequency"):
        be.dedisperse(_fb(), DMS, ref_freq=1593.0)
    with pytest.raises(ValueError, match="int32"):
        Backend.dedisperse_delays(_fb(data=False), [1e9])          # 7.5e8 s of delay x 1e4 Hz
    with pytest.raises(ValueError, match="int32"):
        be.dedisperse(_fb(), [0.0, 1e9])
    with pytest.raises(ValueError, match="fold"):
        be.dedisperse(_fb(fold=True), DMS)
    bb = BasebandSignal(1400, 400, Nchan=2)
    bb._buf = _StubBuf()
    bb._ncols = bb._nsamp = 4096
    with pytest.raises(ValueError, match="FilterBankSignal"):
        be.dedisperse(bb, DMS)
    with pytest.raises(ValueError, match="no data"):
        be.dedisperse(_fb(data=False), DMS)
    # the table's maximum (749) must leave an output sample
    with pytest.raises(ValueError, match="largest delay"):
        be.dedisperse(_fb(n=749), DMS)
    with pytest.raises(ValueError, match="largest delay"):
        be.dedisperse(_fb(n=100), DMS)
    # the plan of a valid call: one sample left
    dm, delays, fref, max_delay, C, N = be._dedisperse_plan(_fb(n=750), DMS)
    assert (max_delay, C, N, fref) == (749, 64, 750, 1593.75)
    assert dm.dtype == np.float64 and np.array_equal(dm, DMS) and delays.dtype == np.int32


def test_cabi_rejections():
    """NULL pointers and each out-of-range scalar return PSS_EINVAL with the
    argument named and no device touched."""
    p = host_pointer()
    # pss_dedisperse(data, nchan, n, ld, delays, ndm, max_delay, out, out_ld, stream)
    good = dict(data=p, nchan=4, n=100, ld=100, delays=p, ndm=3, max_delay=10, out=p, out_ld=90)
    check_rejections(_lib.load().pss_dedisperse, good,
                    ((dict(data=None), "data"), (dict(delays=None), "delays"), (dict(out=None), "out"),
                     (dict(nchan=0), "nchan 0"), (dict(nchan=-3), "nchan -3"),
                     (dict(ndm=0), "ndm 0"), (dict(ndm=-1), "ndm -1"),
                     (dict(ld=99), "ld 99"),
                     (dict(max_delay=-1), "max_delay -1"),
                     (dict(max_delay=100), "max_delay 100"), (dict(max_delay=101, out_ld=0), "max_delay 101"),
                     (dict(n=0, ld=0, max_delay=0), "max_delay 0 >= n 0"),
                     (dict(out_ld=89), "out_ld 89"), (dict(max_delay=0, out_ld=99), "out_ld 99"),
                     # the launch grid: ceil(T / 2048) * ceil(ndm / 8) workgroups in 31 bits
                     (dict(n=1 << 40, ld=1 << 40, out_ld=1 << 40, ndm=64), "workgroups")))
