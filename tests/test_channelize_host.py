"""Host side of the baseband channeliser and the amplitude noise (no GPU):
the prototype filter, every Python-level and C-ABI rejection (nothing reaches
the device), and the host-planned noise scale against the value recorded from
the reference's ``Receiver._make_amp_noise`` (tests/golden/make_bb_noise.py)."""
import numpy as np
import pytest

from psrsigsim_amd import _lib
from tests.fixtures_util import load
from tests.kernel_harness import backend, check_rejections, host_pointer


def _backend():
    return backend(samprate=1.0)


@pytest.mark.parametrize("C,T", [(16, 1), (64, 1), (16, 2), (64, 4), (512, 8), (4096, 3)])
def test_pfb_coefficients(C, T):
    from psrsigsim_amd.telescope import Backend
    h = Backend.pfb_coefficients(C, T)
    L = 2 * C
    assert h.dtype == np.float64 and h.shape == (T * L,)
    assert abs(np.sum(h * h) - L) <= 1e-12 * L
    np.testing.assert_allclose(h, h[::-1], rtol=0, atol=1e-15 * np.max(np.abs(h)))      # symmetric
    if T == 1:
        assert np.all(h == 1.0)
    else:
        i = np.arange(T * L)
        raw = np.sinc((i - (T * L - 1) / 2.0) / L) * np.hamming(T * L)
        np.testing.assert_allclose(h, raw * np.sqrt(L / np.sum(raw ** 2)), rtol=1e-14)
        assert np.argmax(h) in (T * L // 2 - 1, T * L // 2)


class _StubBuf(object):
    """Stands in for the device buffer: any use of it is an error."""

    def __getattr__(self, name):
        raise AssertionError("the device buffer was touched (%s)" % name)


def _bb(npol=2, n=1 << 12, rate=None, data=True):
    from psrsigsim_amd.signal import BasebandSignal
    sig = BasebandSignal(1400, 400, sample_rate=rate, Nchan=npol)
    if data:
        sig._buf = _StubBuf()
        sig._ncols = n
        sig._nsamp = n
    return sig


def test_channelize_rejections_never_reach_the_device(monkeypatch):
    from psrsigsim_amd import _engine
    from psrsigsim_amd.signal import FilterBankSignal

    def boom(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_engine, "to_dev", boom)
    monkeypatch.setattr(_engine, "execute", boom)
    be = _backend()
    with pytest.raises(ValueError, match="BasebandSignal"):
        be.channelize(FilterBankSignal(1400, 400, Nsubband=4, fold=False), 16)
    with pytest.raises(ValueError, match="no data"):
        be.channelize(_bb(data=False), 16)
    with pytest.raises(ValueError, match="sample rate"):
        be.channelize(_bb(rate=1000.0), 16)
    for C in (8, 0, -16, 24, 48, 8192, 4097):
        with pytest.raises(ValueError, match="Nchan"):
            be.channelize(_bb(), C)
    for T in (0, -1, 9):
        with pytest.raises(ValueError, match="ntap"):
            be.channelize(_bb(), 16, ntap=T)
    for ts in (0, -3):
        with pytest.raises(ValueError, match="tscrunch"):
            be.channelize(_bb(), 16, tscrunch=ts)
    with pytest.raises(ValueError, match="polarisation"):
        be.channelize(_bb(npol=3), 16)
    # S < 1: too few samples for one frame, for the taps, for one scrunch group
    with pytest.raises(ValueError, match="no output sample"):
        be.channelize(_bb(n=31), 16)
    with pytest.raises(ValueError, match="no output sample"):
        be.channelize(_bb(n=32 * 4 - 1), 16, ntap=4)
    with pytest.raises(ValueError, match="no output sample"):
        be.channelize(_bb(n=32 * 5), 16, tscrunch=6)
    # the plan of a valid call: (C, T, tscrunch, Npol, N, S)
    assert be._channelize_plan(_bb(n=32 * 20 + 5), 16, 4, 3) == (16, 4, 3, 2, 645, 5)
    assert be._channelize_plan(_bb(npol=1, n=8192 * 3), 4096, 1, 1) == (4096, 1, 1, 1, 24576, 3)


def test_existing_stubs_keep_raising():
    with pytest.raises(NotImplementedError):
        _bb().to_FilterBank()
    assert _backend().adc(_bb()) is None


def test_cabi_rejections():
    """NULL pointers, ld < n, out_ld < S and the parameter ranges return
    PSS_EINVAL with no device touched; S = 0 returns PSS_OK without a launch."""
    L = _lib.load()
    p = host_pointer()
    OK = _lib.PSS_OK
    # pss_channelize(x, npol, n, ld, h, nchan, ntap, tscrunch, out, out_ld, stream)
    good = dict(x=p, npol=2, n=640, ld=640, h=p, nchan=16, ntap=1, tscrunch=1, out=p, out_ld=20)
    big = dict(n=1 << 20, ld=1 << 20, out_ld=1 << 20)
    check_rejections(L.pss_channelize, good,
                     [(dict(x=None), ""), (dict(h=None), ""), (dict(out=None), ""),
                      (dict(ld=639), "ld 639"),                                          # ld < n
                      (dict(out_ld=19), "out_ld 19"),                                    # out_ld < S = 20
                      (dict(ntap=4, tscrunch=3, out_ld=4), "")] +                        # S = (20 - 3) // 3 = 5
                     [(dict(npol=npol), "") for npol in (0, 3, -1)] +
                     [(dict(big, nchan=C), "") for C in (8, 0, -16, 24)] + [(dict(big, nchan=8192), "nchan")] +
                     [(dict(ntap=T), "") for T in (0, 9, -2)] +
                     [(dict(tscrunch=0), ""), (dict(n=-1), "")])
    # nothing to do: no whole frame, fewer frames than taps, no whole scrunch group
    assert L.pss_channelize(p, 2, 31, 31, p, 16, 1, 1, p, 0, None) == OK
    assert L.pss_channelize(p, 1, 32 * 7, 32 * 7, p, 16, 8, 1, p, 0, None) == OK
    assert L.pss_channelize(p, 2, 32 * 5, 32 * 5, p, 16, 1, 6, p, 0, None) == OK
    assert L.pss_channelize(p, 2, 0, 0, p, 4096, 1, 1, p, 0, None) == OK
    # pss_normal_add(rows, nrows, n, ld, scale, seed, call_id, stream)
    good = dict(rows=p, nrows=2, n=100, ld=100, scale=1.0, seed=1, call_id=1)
    check_rejections(L.pss_normal_add, good, ((dict(rows=None), ""), (dict(ld=99), "ld 99"),          # ld < n
                                              (dict(nrows=65536), ""), (dict(n=-1), "")))
    assert L.pss_normal_add(p, 0, 100, 100, 1.0, 1, 1, None) == OK                        # no rows
    assert L.pss_normal_add(p, 2, 0, 100, 1.0, 1, 1, None) == OK                          # no samples


def test_header_declares_and_binding_exports_the_new_entries():
    from tests.test_cabi import header_functions
    names = header_functions()
    for n in ("pss_channelize", "pss_normal_add"):
        assert n in names and n in _lib.EXPORTS and hasattr(_lib.load(), n)


def test_new_unit_is_hashed_into_the_build():
    from psrsigsim_amd import build
    assert "pss_channelize.hip" in build.UNITS
    assert any(d.endswith("pss_channelize.hip") for d in build.DEPS)


@pytest.mark.parametrize("tag", ["bb_obs", "small"])
def test_amp_noise_norm_matches_the_reference(tag):
    """Our float64 host plan of receiver.py:126-135's ``norm`` against the
    value the unmodified reference returned with its draws replaced by ones."""
    from psrsigsim_amd.signal import BasebandSignal
    from psrsigsim_amd.pulsar import Pulsar
    from psrsigsim_amd.telescope import Receiver
    from psrsigsim_amd.utils import make_quant
    meta, A, _ = load("bb_noise")
    g = meta["geoms"][tag]
    sig = BasebandSignal(g["fcent"], g["bw"], sample_rate=g["sample_rate"], Nchan=2)
    psr = Pulsar(g["period"], g["Smean"], name="J1746-0118")
    psr.make_pulses(sig, g["tobs"])
    assert sig.nsamp == g["nsamp"] and sig._samprate_MHz() == g["samprate_MHz"]
    rcvr = Receiver(fcent=g["fcent"], bandwidth=g["bw"], name="Lband")
    Tsys = rcvr.Trec if g["Tsys"] is None else make_quant(g["Tsys"], "K")
    norm = Receiver.amp_noise_norm(sig, psr, Tsys, make_quant(g["gain"], "K/Jy"))
    assert norm == pytest.approx(g["norm"], rel=1e-12)
    assert A["norm_" + tag][0] == g["norm"]
