"""Search-mode PSRFITS output, the parts that need no device: constructing the
writer, the argument checks that come before any GPU work, ``read_search_data``
on a file assembled by hand (known codes at 8, 4 and 2 bits: the codes, the
values code * DAT_SCL + DAT_OFFS and the channel order inside a byte), and
the C ABI's rejections through ctypes (as tests/test_cabi.py does)."""
import os

import numpy as np
import pytest

from psrsigsim_amd import _lib
from psrsigsim_amd._units import Quantity
from psrsigsim_amd.io import PSRFITS, read_search_data
from psrsigsim_amd.io.psrfits import _card, _header
from tests.kernel_harness import check_rejections, host_pointer

TEMPLATE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data",
                        "B1855+09.L-wide.PUPPI.11y.x.sum.sm")


class _FakeSig(object):
    def __init__(self, nchan, nsamp):
        self.Nchan = nchan
        self.samprate = Quantity(0.05, "MHz")
        self.tobs = Quantity(nsamp / 0.05e6, "s")
        self.sublen = None
        self.fcent = Quantity(430.0, "MHz")
        self.bw = Quantity(100.0, "MHz")
        self.dat_freq = Quantity(380.0 + np.arange(nchan) * 100.0 / nchan, "MHz")
        self.dm = Quantity(10.0, "pc/cm^3")
        self.data = np.zeros((nchan, nsamp), dtype=np.float32)
        self.nsamp = nsamp
        self.Npols = 1


class _FakePsr(object):
    name = "J0000+0000"
    period = Quantity(1.0, "s")


def test_search_mode_constructs(tmp_path):
    pf = PSRFITS(str(tmp_path / "s.fits"), obs_mode="SEARCH")
    assert pf.obs_mode == "SEARCH"


def test_search_mode_with_template_still_unsupported(tmp_path):
    """The template copy is the reference's fold-only path."""
    with pytest.raises(NotImplementedError):
        PSRFITS(str(tmp_path / "s.fits"), obs_mode="SEARCH", template=TEMPLATE)
    with pytest.raises(NotImplementedError):
        PSRFITS(str(tmp_path / "s.fits"), obs_mode="BOGUS")


@pytest.mark.parametrize("nchan,kw", [(4, dict(nbits=3)), (3, dict(nbits=4)), (4, dict(nsblk=4096))])
def test_save_rejects_bad_geometry_before_any_device_use(tmp_path, monkeypatch, nchan, kw):
    """nbits = 3, three channels at 4 bits (12 bits: no whole byte), and an
    nsblk larger than the data (no whole row) raise ValueError; the device
    helpers are never reached."""
    from psrsigsim_amd import _engine

    def boom(*a, **k):
        raise AssertionError("device use before the argument checks")
    monkeypatch.setattr(_engine, "to_dev", boom)
    monkeypatch.setattr(_engine, "device", boom)
    monkeypatch.setattr(_lib, "lib", boom)
    path = tmp_path / "s.fits"
    with pytest.raises(ValueError):
        PSRFITS(str(path), obs_mode="SEARCH").save(_FakeSig(nchan, 100), _FakePsr(), **kw)
    assert not path.exists()


def _pack(codes, nbits):
    """codes [nrows][nsblk][nchan] -> bytes [nrows][nsblk][nchan nbits / 8],
    the lower-numbered channel in the more significant bits of its byte
    (written out per bit depth, independently of the reader's loop)."""
    c = codes.astype(np.uint8)
    if nbits == 8:
        return c
    if nbits == 4:
        return (c[..., 0::2] << 4) | c[..., 1::2]
    return (c[..., 0::4] << 6) | (c[..., 1::4] << 4) | (c[..., 2::4] << 2) | c[..., 3::4]


def _write_by_hand(path, packed, scl, offs, nbits, nchan, nsblk):
    nrows = packed.shape[0]
    nb = nchan * nbits // 8
    row = np.dtype([("TSUBINT", ">f8"), ("DAT_OFFS", ">f4", (nchan,)), ("DAT_SCL", ">f4", (nchan,)),
                    ("DATA", "u1", (nsblk * nb,))])
    tab = np.zeros(nrows, dtype=row)
    tab["TSUBINT"] = 1.0
    tab["DAT_OFFS"] = offs
    tab["DAT_SCL"] = scl
    tab["DATA"] = packed.reshape(nrows, -1)
    prim = [_card("SIMPLE", True), _card("BITPIX", 8), _card("NAXIS", 0), _card("EXTEND", True),
            _card("OBS_MODE", "SEARCH")]
    sub = [_card("XTENSION", "BINTABLE"), _card("BITPIX", 8), _card("NAXIS", 2), _card("NAXIS1", row.itemsize),
           _card("NAXIS2", nrows), _card("PCOUNT", 0), _card("GCOUNT", 1), _card("TFIELDS", 4),
           _card("TTYPE1", "TSUBINT"), _card("TFORM1", "1D"),
           _card("TTYPE2", "DAT_OFFS"), _card("TFORM2", "%dE" % nchan),
           _card("TTYPE3", "DAT_SCL"), _card("TFORM3", "%dE" % nchan),
           _card("TTYPE4", "DATA"), _card("TFORM4", "%dB" % (nsblk * nb)),
           _card("TDIM4", "(1,%d,1,%d)" % (nb, nsblk)),
           _card("EXTNAME", "SUBINT"), _card("NPOL", 1), _card("NCHAN", nchan), _card("NSBLK", nsblk),
           _card("NBITS", nbits)]
    body = tab.tobytes()
    with open(path, "wb") as f:
        f.write(_header(prim))
        f.write(_header(sub))
        f.write(body + b"\0" * ((-len(body)) % 2880))


@pytest.mark.parametrize("nbits", [8, 4, 2])
def test_read_search_data_hand_assembled(tmp_path, nbits):
    nrows, nsblk, nchan = 2, 3, 4
    L = (1 << nbits) - 1
    # known codes: every level reachable in 24 samples, 0 and L included
    codes = ((np.arange(nrows * nsblk * nchan) * 7 + 3) % (L + 1)).reshape(nrows, nsblk, nchan)
    codes[0, 0, 0], codes[1, 2, 3] = 0, L
    scl = np.array([[0.5, 0.25, 2.0, 1.0], [3.0, 0.125, 1.5, 1.0]], dtype=np.float32)
    offs = np.array([[-1.0, 0.0, 10.0, 0.5], [2.0, -8.0, 0.25, 100.0]], dtype=np.float32)
    packed = _pack(codes, nbits)
    assert packed.shape == (nrows, nsblk, nchan * nbits // 8)
    if nbits == 4:                                   # channel 2k in the high nibble
        assert packed[0, 1, 0] == (codes[0, 1, 0] << 4 | codes[0, 1, 1])
    path = str(tmp_path / ("hand%d.fits" % nbits))
    _write_by_hand(path, packed, scl, offs, nbits, nchan, nsblk)
    got_codes, got_vals, prim, sub = read_search_data(path)
    assert got_codes.dtype == np.uint8 and got_codes.shape == (nchan, nrows * nsblk)
    assert got_vals.dtype == np.float32 and got_vals.shape == got_codes.shape
    want_codes = codes.reshape(nrows * nsblk, nchan).T
    np.testing.assert_array_equal(got_codes, want_codes)
    # (these scales and offsets are dyadic: code * scl + offs is exact in float32)
    want_vals = (codes * scl[:, None, :].astype(np.float64) + offs[:, None, :]).reshape(nrows * nsblk, nchan).T
    np.testing.assert_array_equal(got_vals, want_vals.astype(np.float32))
    assert (want_vals.astype(np.float32) == want_vals).all()
    assert prim["OBS_MODE"] == "SEARCH" and sub["NBITS"] == nbits and sub["NSBLK"] == nsblk


def test_cabi_rejections():
    """NULL pointers, ld too small, nbits = 3 and a channel count that does
    not fill whole bytes return PSS_EINVAL with no device touched; work of
    size zero returns PSS_OK without a launch."""
    L = _lib.load()
    p = host_pointer()
    # pss_chan_stats(data, nchan, ld, nsblk, nrows, mn, mx, sum, sumsq, stream)
    good = dict(data=p, nchan=2, ld=100, nsblk=10, nrows=2, mn=p, mx=p, sum=p, sumsq=p)
    check_rejections(L.pss_chan_stats, good,
                     ((dict(data=None), ""), (dict(mn=None), ""), (dict(sumsq=None), ""),
                      (dict(ld=19), "ld 19"),                                     # ld < nrows * nsblk
                      (dict(nsblk=0), ""),                                        # nsblk < 1
                      (dict(nchan=65536), "")))
    assert L.pss_chan_stats(p, 2, 100, 10, 0, p, p, p, p, None) == _lib.PSS_OK    # no rows
    assert L.pss_chan_stats(p, 0, 100, 10, 2, p, p, p, p, None) == _lib.PSS_OK    # no channels
    # pss_quantize_tmajor(data, nchan, ld, nsblk, nrows, scl, offs, nbits, out, stream)
    good = dict(data=p, nchan=2, ld=100, nsblk=10, nrows=2, scl=p, offs=p, nbits=8, out=p)
    check_rejections(L.pss_quantize_tmajor, good,
                     ((dict(data=None), ""), (dict(scl=None), ""), (dict(offs=None), ""), (dict(out=None), ""),
                      (dict(ld=19), ""),                                          # ld < nrows * nsblk
                      (dict(nbits=3), "nbits 3"), (dict(nbits=16), ""),
                      (dict(nchan=3, nbits=4), ""),                               # 12 bits per sample
                      (dict(nchan=2, nbits=2), "whole bytes"),                    # 4 bits per sample
                      (dict(nsblk=0), ""),                                        # nsblk < 1
                      (dict(nchan=65536), "")))
    assert L.pss_quantize_tmajor(p, 2, 100, 10, 0, p, p, 8, p, None) == _lib.PSS_OK


def test_header_declares_and_binding_exports_the_new_entries():
    from tests.test_cabi import header_functions
    names = header_functions()
    for n in ("pss_chan_stats", "pss_quantize_tmajor"):
        assert n in names and n in _lib.EXPORTS and hasattr(_lib.load(), n)


def test_new_unit_is_hashed_into_the_build():
    from psrsigsim_amd import build
    assert "pss_searchout.hip" in build.UNITS
    assert any(d.endswith("pss_searchout.hip") for d in build.DEPS)
