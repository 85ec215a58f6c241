"""Host side of the spectrum whitening (no GPU): the planner
``Backend.whiten_plan`` against the restatement, the restatement's own
properties (tests/whiten_ref.py), every ValueError of the planner, the mask
builder and the new keywords, the C ABI's argument checks, which precede any
launch, and the mask ``Backend.zap_mask``."""
import os
import re

import numpy as np
import pytest

from psrsigsim_amd import _lib
from tests import whiten_ref as ref
from tests.kernel_harness import check_rejections, host_pointer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NBINS = (1, 2, 5, 6, 7, 11, 12, 13, 48, 49, 1023, 1024, 1025, 2047, 16384)
WIDTHS = ((1, 1), (6, 128), (128, 128), (2, 3))


def _Backend():
    from psrsigsim_amd.telescope import Backend
    return Backend


# ---------------------------------------------------------------------------
# the planner
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("w0,wmax", WIDTHS)
def test_plan_is_the_restatement_and_keeps_its_invariants(w0, wmax):
    from psrsigsim_amd.telescope import WhitenPlan
    B = _Backend()
    done = 0
    for nbin in NBINS:
        for kstart in (0, 1, 5):
            if kstart >= nbin:
                with pytest.raises(ValueError, match="whiten_plan: kstart"):
                    B.whiten_plan(nbin, kstart, w0, wmax)
                continue
            p = B.whiten_plan(nbin, kstart=kstart, w0=w0, wmax=wmax)
            assert isinstance(p, WhitenPlan)
            e = p.edges
            assert e.dtype == np.int64 and np.array_equal(e, ref.plan_ref(nbin, kstart, w0, wmax))
            assert (p.nbin, p.kstart, p.w0, p.wmax, p.nblk) == (nbin, kstart, w0, wmax, e.size - 1)
            w = np.diff(e)
            assert e[0] == kstart and e[-1] == nbin and w.min() >= 1 and w.max() <= 255
            assert w.max() < 2 * wmax
            # the planned width from 8 wmax on (the last block alone may be longer)
            flat = np.flatnonzero(e[:-2] >= 8 * wmax)
            assert np.all(w[flat] == wmax)
            done += 1
    assert done >= 40


def test_default_plan_at_scale():
    """2^19 bins: 4 086 blocks of 128 (the bins from 1024 on) against 35
    narrower ones -- 8 of 6 bins up to bin 48, then e -> e + e / 8, about
    ln(1024 / 48) / ln(9 / 8) = 26 more -- and the last, longer one."""
    p = _Backend().whiten_plan(1 << 19)
    w = np.diff(p.edges)
    assert (p.kstart, p.w0, p.wmax) == (1, 6, 128) and w[0] == 6
    assert int((w == 128).sum()) == 4086 and int((w < 128).sum()) == 35 and w[-1] == 202 and p.nblk == 4122


# ---------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------
def _noise(ndm, nbin, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((ndm, nbin, 2)) * np.sqrt(0.5)
    return (x[..., 0] + 1j * x[..., 1]).astype(np.complex64)


def test_whitened_noise_has_unit_mean_power():
    """Unit-mean exp(1) powers under a smooth factor of 100 over the band:
    above bin 64 the whitened power has a mean within 5 % of 1."""
    nbin = 16384
    k = np.arange(nbin)
    for seed in (1, 2, 3):
        x = _noise(2, nbin, seed) * np.sqrt(100.0 ** (1.0 - k / nbin)).astype(np.float32)
        raw = ref.power(x)
        assert raw[:, :1024].mean() > 50 * raw[:, -1024:].mean()
        edges = ref.plan_ref(nbin)
        P = ref.power(ref.whiten_ref(x, edges))
        for j in range(2):
            m = float(P[j, 64:].astype(np.float64).mean())
            print("seed %d trial %d: whitened mean power %.4f" % (seed, j, m))
            assert abs(m - 1.0) < 0.05
        assert not P[:, 0].any()                                   # below kstart


def test_single_block_and_zero_row():
    x = _noise(2, 200, 4)
    x[1] = 0                                                       # a zero-padded row
    edges = np.array([0, 200], dtype=np.int64)
    med = ref.medians_ref(x, edges)
    assert med.shape == (2, 1)
    assert med[0, 0] == np.sort(ref.power(x[0]))[99] and med[1, 0] == 0
    out = ref.whiten_ref(x, edges)
    s = np.sqrt(ref.LN2_F32 / med[0, 0])
    assert s.dtype == np.float32
    assert np.array_equal(out[0].real, x[0].real * s) and np.array_equal(out[0].imag, x[0].imag * s)
    assert not out[1].real.any() and not out[1].imag.any()         # s = 0: all zeros
    # interpolation runs from centre to centre and is flat outside
    edges = np.array([2, 6, 10], dtype=np.int64)
    n = ref.norm_ref(np.array([[1.0, 3.0]], dtype=np.float32), edges, 10)[0]
    assert np.array_equal(n[:4], [1, 1, 1, 1]) and np.array_equal(n[8:], [3, 3])
    assert np.array_equal(n[4:8], np.float32(1) + np.float32(2) * (np.array([1, 3, 5, 7], dtype=np.float32)
                                                                    / np.float32(8)))
    z = np.zeros(10, dtype=np.uint8)
    z[[1, 7]] = 1
    out = ref.whiten_ref(_noise(1, 10, 5), edges, zap=z)
    assert out[0, 0] == 0 and out[0, 1] == 0 and out[0, 7] == 1    # below edges[0] first, then the mask
    # NaN keys sort last and come out canonical
    x = _noise(1, 8, 6)
    x[0, :5] = np.nan
    m = ref.medians_ref(x, np.array([0, 8], dtype=np.int64))       # sorted index 3 of 8 with 5 NaN
    assert m.view(np.uint32)[0, 0] == 0x7FC00000


# ---------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------
def test_whiten_plan_rejections():
    B = _Backend()
    for kw, word in ((dict(nbin=0), "nbin 0 < 1"), (dict(nbin=10.5), "integers"), (dict(w0=0), "w0 0"),
                     (dict(w0=7, wmax=6), "w0 7 and wmax 6"), (dict(wmax=129), "wmax 129"),
                     (dict(kstart=-1), "kstart -1"), (dict(kstart=100), "kstart 100"), (dict(w0="a"), "integers")):
        args = dict(nbin=100, kstart=1, w0=6, wmax=128)
        args.update(kw)
        with pytest.raises(ValueError, match="whiten_plan: .*" + re.escape(word)):
            B.whiten_plan(**args)


def test_zap_mask_and_its_rejections():
    B = _Backend()
    nfft, fs_MHz = 1000, 0.002                                     # df = 2 Hz, bins 0 .. 499 at 0 .. 998 Hz
    ranges = [(59.0, 61.0), (120.0, 124.0), (0.0, 0.0), (2000.0, 3000.0), (996.5, 5000.0), (301.0, 301.9)]
    m = B.zap_mask(nfft, fs_MHz, ranges)
    assert m.dtype == np.uint8 and m.shape == (500,)
    assert np.array_equal(m, ref.zap_mask_ref(nfft, fs_MHz * 1e6, ranges))
    # closed ranges: 120 and 124 Hz are bin centres; the range above the band and the one between centres set nothing
    assert np.array_equal(np.flatnonzero(m), [0, 30, 60, 61, 62, 499])
    # quantities go through to_value
    from psrsigsim_amd._units import make_quant
    mq = B.zap_mask(nfft, make_quant(2.0, "kHz"), [(make_quant(0.059, "kHz"), make_quant(61.0, "Hz"))])
    assert np.array_equal(np.flatnonzero(mq), [30])
    assert not B.zap_mask(nfft, fs_MHz, []).any()
    for args, word in (((1001, fs_MHz, []), "nfft 1001"), ((0, fs_MHz, []), "nfft 0"), ((nfft, 0.0, []), "sample rate"),
                       ((nfft, np.nan, []), "sample rate"), ((nfft, fs_MHz, [(2.0, 1.0)]), "range"),
                       ((nfft, fs_MHz, [(1.0,)]), "range"), ((nfft, fs_MHz, [(np.nan, 1.0)]), "range"),
                       ((nfft, fs_MHz, [5.0]), "range"), ((nfft, fs_MHz, 7), "range"),
                       ((10.5, fs_MHz, []), "integers")):
        with pytest.raises(ValueError, match="zap_mask: .*" + word):
            B.zap_mask(*args)


def test_keyword_rejections_touch_no_device():
    from psrsigsim_amd.telescope import DedispersedPlane

    class Stub(object):
        shape = (3, 4096)

        def __getattr__(self, name):
            raise AssertionError("the device buffer was touched (%s)" % name)

    import torch
    B = _Backend()
    be = B(samprate=0.01)
    plane = DedispersedPlane(Stub(), np.arange(3.0), None, 0.01, 1400.0, 0)
    nbin = 2048
    mask = np.zeros(nbin, dtype=np.uint8)
    calls = (lambda **kw: be.harmonic_snr(plane, **kw), lambda **kw: be.periodicity_search(plane, **kw),
             lambda **kw: be.accel_snr(plane, [0.0], **kw), lambda **kw: be.accel_search(plane, accels=[0.0], **kw),
             lambda **kw: B._harmonic_plan(plane, **kw))
    for call in calls:
        for kw in (dict(zap=mask), dict(zap=mask, whiten=None), dict(zap=mask, whiten=False)):
            with pytest.raises(ValueError, match="zap needs whiten"):
                call(**kw)
        with pytest.raises(ValueError, match="whiten must be"):
            call(whiten="yes")
        with pytest.raises(ValueError, match="whiten holds width"):
            call(whiten=dict(width=3))
        with pytest.raises(ValueError, match="whiten_plan: .*wmax 200"):
            call(whiten=dict(wmax=200))
        with pytest.raises(ValueError, match="edges"):
            call(whiten=B.whiten_plan(nbin - 1))                   # a plan for another length
        with pytest.raises(ValueError, match="zap"):
            call(whiten=True, zap=mask[:-1])
        with pytest.raises(ValueError, match="zap"):
            call(whiten=True, zap=np.zeros(nbin))                  # not a mask of integers
        with pytest.raises(ValueError, match="zap has the shape"):
            call(whiten=True, zap=torch.zeros(nbin - 1, dtype=torch.uint8))      # a tensor (here on the host)
        with pytest.raises(ValueError, match="zap has the shape"):
            call(whiten=True, zap=torch.zeros((1, nbin), dtype=torch.uint8))
    # what the plan resolves to
    p = B._harmonic_plan(plane)
    assert p["whiten"] is None and p["zap"] is None
    p = B._harmonic_plan(plane, whiten=True, zap=mask.astype(bool))
    assert np.array_equal(p["whiten"].edges, ref.plan_ref(nbin)) and p["zap"].dtype == np.uint8
    p = B._harmonic_plan(plane, whiten=dict(kstart=3, wmax=64))
    assert np.array_equal(p["whiten"].edges, ref.plan_ref(nbin, 3, 6, 64))
    own = B.whiten_plan(nbin, w0=2, wmax=3)
    assert B._harmonic_plan(plane, whiten=own)["whiten"] is own
    # a hand-made table is checked on the host
    from psrsigsim_amd.telescope import WhitenPlan
    for edges in ([0, 300, nbin], [0, 10, 10, nbin], [-1, 100, nbin], [0, 100], [[0, nbin]], [0.0, float(nbin)]):
        bad = WhitenPlan(np.array(edges), nbin, 0, 1, 128)
        with pytest.raises(ValueError, match="edges"):
            B._harmonic_plan(plane, whiten=bad)
    for fn in (be.spectrum_medians, be.whiten_spectrum):
        with pytest.raises(ValueError, match="spectrum"):
            fn(np.zeros((2, 9), dtype=np.complex64))
    from psrsigsim_amd.telescope import HarmonicPlane, AccelPlane
    assert HarmonicPlane.whiten is None and AccelPlane.whiten is None


# ---------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_hashed():
    from psrsigsim_amd import build
    with open(os.path.join(ROOT, "include", "pss_hip.h")) as f:
        header = f.read()
    for name, nargs in (("pss_spectrum_medians", 9), ("pss_spectrum_whiten", 12)):
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
        assert len(_lib.EXPORTS[name][1]) == nargs and hasattr(_lib.load(), name)
    assert "pss_whiten.hip" in build.UNITS and any(d.endswith("pss_whiten.hip") for d in build.DEPS)


def test_entry_points_validate_arguments():
    """Every PSS_EINVAL of the two entry points with NULL or host pointers:
    the checks precede any launch (no GPU touched)."""
    import ctypes
    p = host_pointer()
    L = _lib.load()
    big = (1 << 31) - 1
    common = ((dict(spec=None), "spec is NULL"), (dict(edges=None), "edges is NULL"), (dict(med=None), "med is NULL"),
              (dict(ndm=0), "ndm 0 < 1"), (dict(nbin=0, ld=0), "nbin 0 < 1"), (dict(nblk=0), "nblk 0 < 1"),
              (dict(nblk=-3), "nblk -3 < 1"), (dict(nblk=17, med_ld=17), "nblk 17 > nbin 16"),
              (dict(ld=15), "ld 15 < nbin 16"), (dict(med_ld=3), "med_ld 3 < nblk 4"))
    good = dict(spec=p, ndm=2, nbin=16, ld=16, edges=p, nblk=4, med=p, med_ld=4)
    check_rejections(L.pss_spectrum_medians, good, common + (
        (dict(nbin=big, ld=big, nblk=big, med_ld=big, ndm=64),
         "67108864 block groups x 64 trials exceed 2^31 - 1 workgroups"),), prefix="spectrum_medians: ")
    good = dict(good, zap=None, out=p, out_ld=16)
    other = ctypes.c_void_p(p.value + 64)                          # inside the rows of spec
    far = ctypes.c_void_p(p.value + (1 << 20))
    check_rejections(L.pss_spectrum_whiten, good, common + (
        (dict(out=None), "out is NULL"), (dict(out_ld=15), "out_ld 15 < nbin 16"),
        (dict(out_ld=17), "out overlaps spec"), (dict(out=other), "out overlaps spec"),
        (dict(out=far, nbin=1 << 40, ld=1 << 40, out_ld=1 << 40), "out overlaps spec"),
        (dict(nbin=1 << 40, ld=1 << 40, out_ld=1 << 40, ndm=4),
         "1073741824 bin tiles x 4 trials exceed 2^31 - 1 workgroups")), prefix="spectrum_whiten: ")

