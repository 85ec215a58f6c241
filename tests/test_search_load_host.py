"""Search-mode PSRFITS input, the parts that need no device: the argument
checks of ``pss_unpack_tmajor`` through ctypes, its declaration and build
entries, the files ``load_search_signal`` refuses before any device use, and
the file helper of tests/search_load_ref.py against ``read_search_data``."""
import numpy as np
import pytest

from psrsigsim_amd import _lib
from psrsigsim_amd.io import PSRFITS, load_search_signal, read_search_data
from tests.kernel_harness import check_rejections, host_pointer
from tests.search_load_ref import random_case, unpack_ref, write_search_file


def test_cabi_rejections_and_noops():
    L = _lib.load()
    p = host_pointer()
    # pss_unpack_tmajor(in, nchan, npol, nsum, nsblk, nrows, scl, offs, wts, zero_off, nbits, flip, out, ld, stream)
    good = dict(inp=p, nchan=2, npol=1, nsum=1, nsblk=10, nrows=2, scl=p, offs=p, wts=None, zero_off=0.0, nbits=8,
                flip=0, out=p, ld=100)
    check_rejections(L.pss_unpack_tmajor, good,
                     ((dict(inp=None), "NULL"), (dict(scl=None), "NULL"), (dict(offs=None), "NULL"),
                      (dict(out=None), "NULL"),
                      (dict(nbits=3), "nbits 3"), (dict(nbits=16), "nbits 16"), (dict(nbits=1), "nbits 1"),
                      (dict(npol=3), "npol 3"), (dict(npol=0), "npol 0"),
                      (dict(nsum=0), "nsum 0"), (dict(nsum=3, npol=4), "nsum 3"), (dict(nsum=2, npol=1), "nsum 2"),
                      (dict(nchan=3, nbits=4), "whole bytes"), (dict(nchan=2, nbits=2), "whole bytes"),
                      (dict(nsblk=0), "nsblk 0"),
                      (dict(ld=19), "ld 19"),                                      # ld < nrows * nsblk
                      (dict(nchan=65536), "65535")))
    assert L.pss_unpack_tmajor(p, 2, 1, 1, 10, 0, p, p, None, 0.0, 8, 0, p, 100, None) == _lib.PSS_OK    # no rows
    assert L.pss_unpack_tmajor(p, 0, 1, 1, 10, 2, p, p, None, 0.0, 8, 0, p, 100, None) == _lib.PSS_OK    # no channels


def test_header_declares_and_binding_exports_the_entry():
    from tests.test_cabi import header_functions
    assert "pss_unpack_tmajor" in header_functions()
    assert "pss_unpack_tmajor" in _lib.EXPORTS and hasattr(_lib.load(), "pss_unpack_tmajor")


def test_new_unit_is_hashed_into_the_build():
    from psrsigsim_amd import build
    assert "pss_searchin.hip" in build.UNITS
    assert any(d.endswith("pss_searchin.hip") for d in build.DEPS)


def _file(path, nbits=8, nchan=8, nsblk=4, nrows=3, npol=1, freq=None, **kw):
    codes, scl, offs = random_case(nbits, nchan, nsblk, nrows, npol=npol)
    freq = 1200.0 + 50.0 * np.arange(nchan) if freq is None else freq
    write_search_file(str(path), codes, scl, offs, np.ones((nrows, nchan)), freq, nbits, **kw)
    return codes, scl, offs


REFUSED = [
    ("nbits16", dict(cards=(("NBITS", 16),)), NotImplementedError, "16"),
    ("signint", dict(cards=(("SIGNINT", 1),)), NotImplementedError, "SIGNINT"),
    ("nbin2", dict(cards=(("NBIN", 2),)), NotImplementedError, "NBIN = 2"),
    ("poltype", dict(npol=4, pol_type="XXYY?"), NotImplementedError, "XXYY?"),
    ("zigzag", dict(freq=np.array([1200.0, 1250.0, 1225.0, 1300.0, 1350.0, 1400.0, 1450.0, 1500.0])), ValueError,
     "monotonic"),
    ("rows_behind", dict(rows=(2, 4)), ValueError, "rows"),
    ("rows_empty", dict(rows=(1, 1)), ValueError, "rows"),
    ("rows_negative", dict(rows=(-1, 2)), ValueError, "rows"),
]


@pytest.mark.parametrize("name,kw,exc,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_loader_refuses_before_any_device_use(tmp_path, monkeypatch, name, kw, exc, word):
    from psrsigsim_amd import _engine

    def boom(*a, **k):
        raise AssertionError("device use before the checks")
    monkeypatch.setattr(_engine, "to_dev", boom)
    monkeypatch.setattr(_engine, "device", boom)
    monkeypatch.setattr(_lib, "lib", boom)
    kw = dict(kw)
    rows = kw.pop("rows", None)
    path = tmp_path / (name + ".fits")
    _file(path, **kw)
    with pytest.raises(exc, match=word.replace("?", r"\?")):
        load_search_signal(str(path), rows=rows)
    with pytest.raises(exc):
        PSRFITS(str(path)).load_search(rows=rows)


def test_loader_refuses_frequencies_that_change_between_rows(tmp_path):
    freq = np.tile(1200.0 + 50.0 * np.arange(8), (3, 1))
    freq[2, 5] += 1.0
    path = tmp_path / "rows_differ.fits"
    _file(path, freq=freq)
    with pytest.raises(ValueError, match="differs between rows"):
        load_search_signal(str(path))


@pytest.mark.parametrize("nbits", [8, 4, 2])
def test_file_helper_against_read_search_data(tmp_path, nbits):
    """The helper's NPOL 1 file read back by the package's host reader: the
    same codes, and the restatement's values rounded to float32."""
    path = tmp_path / "helper.fits"
    codes, scl, offs = _file(path, nbits=nbits, nchan=12, nsblk=5, nrows=3)
    got_codes, got_vals, prim, sub = read_search_data(str(path))
    np.testing.assert_array_equal(got_codes, codes[:, :, 0, :].reshape(15, 12).T)
    ref, _ = unpack_ref(codes, scl, offs)
    np.testing.assert_array_equal(got_vals, ref.astype(np.float32))
    assert prim["OBS_MODE"] == "SEARCH" and sub["NBITS"] == nbits and sub["NSBLK"] == 5 and sub["NPOL"] == 1
