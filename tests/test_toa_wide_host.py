"""Host side of the wideband arrival-time stage (no GPU): the float64 model of
``pss_toa_wide_fit`` (tests/toa_wide_ref.py) on noise-free portraits, in a
Monte-Carlo of its error bars and at low signal where the per-channel fit
fails; that the inputs of the GPU tests converge and keep clear of near-tied
peaks under the model alone; the planner, ``WidebandTOAs`` and its ``.tim``
output; the C ABI's argument checks (they precede any launch)."""
import os
import re
from decimal import Decimal

import numpy as np
import pytest

from psrsigsim_amd import _lib
from tests import toa_ref as ref
from tests import toa_wide_ref as wref
from tests.kernel_harness import check_rejections, host_pointer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _Backend():
    from psrsigsim_amd.telescope import Backend
    return Backend


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ndm", (1, 5))
@pytest.mark.parametrize("nbin", (256, 97, 2048))
def test_model_returns_the_injected_phase_and_dm(nbin, ndm):
    """Noise-free portraits b_n s(phi - phi0_n - phi - kappa_n d), s rebuilt
    from the rounded table so that the table is exact for them: phi to 1e-9
    turns (circular) and d to 1e-9 / (kappa's span), with phi over [-1/2, 1/2)
    and at the wrap, d a few bins across the band off the start (ndm = 1) or
    between the trials (ndm = 5)."""
    nchan = 7
    kappa = wref.band(nchan)
    span = kappa.max() - kappa.min()
    step = wref.dm_step_half_bin(kappa, nbin) if ndm > 1 else 0.0
    e = 1.0 / nbin
    phis = np.concatenate([np.linspace(-0.5, 0.5, 11, endpoint=False), [-0.5 + 0.3 * e, 0.5 - 0.3 * e, 0.5 - 1e-7,
                                                                         0.3 * e, -0.99 * e]])
    rng = np.random.default_rng([nbin, ndm])
    if ndm > 1:
        ds = rng.uniform(-0.48, 0.48, phis.size) * ndm * step
    else:
        ds = rng.uniform(-3.0, 3.0, phis.size) * e / span
    phi0 = ref.circ(rng.uniform(-0.5, 0.5, nchan))
    for nharm in (nbin, max(4, nbin // 8)):
        s, spec = ref.band_limited(ref.make_template(nbin), nharm)
        prof = np.empty((nchan, phis.size, nbin))
        for i, (phi, d) in enumerate(zip(phis, ds)):
            prof[:, i] = ref.shifted(s, phi0 + phi + kappa * d, 1.0 + 0.1 * np.arange(nchan), 0.3)
        o, p = wref.wide_ref(prof, spec[None], nharm, kappa, phi0, np.ones((nchan, phis.size), np.float32), ndm, step)
        dphi = np.abs(ref.circ(o[:, wref.PHI] - phis)).max()
        dd = np.abs(o[:, wref.D] - ds).max() * span
        print("nbin %d ndm %d nharm %d: |phi - phi0| max %.3g, |d - d0| x span max %.3g, evaluations max %d"
              % (nbin, ndm, nharm, dphi, dd, o[:, wref.NEV].max()))
        assert not o[:, wref.STATUS].any()
        assert dphi <= 1e-9 and dd <= 1e-9
        assert (o[:, wref.PHI] >= -0.5).all() and (o[:, wref.PHI] < 0.5).all()
        assert np.abs(p[:, :, 0] / (1.0 + 0.1 * np.arange(nchan))[:, None] - 1).max() <= 1e-9 and (p[:, :, 3] == 1).all()


def test_model_error_bars_in_a_monte_carlo():
    """1000 draws of Gaussian noise on 16 channels of 256 bins at b / b_err =
    30 per channel: the pulls of phi and of d have |mean| <= 5 / sqrt(n) and a
    standard deviation within 1 +- 5 / sqrt(2 n); the mean of chi2r lies within
    5 of its own standard deviations, sqrt(2 / (dof n)), of 1."""
    n = 1000
    c = wref.low_signal(n, snr=30.0, seed=7)
    o, _ = wref.wide_ref(*wref.model_args(c))
    assert not o[:, wref.STATUS].any()
    pp = ref.circ(o[:, wref.PHI] - c["phi"]) / o[:, wref.PHI_ERR]
    pd = (o[:, wref.D] - c["d"]) / o[:, wref.D_ERR]
    chi2r = o[:, wref.CHI2] / o[:, wref.DOF]
    print("phi pull mean %.4f std %.4f; d pull mean %.4f std %.4f; chi2r mean %.5f (dof %d); evaluations max %d"
          % (pp.mean(), pp.std(), pd.mean(), pd.std(), chi2r.mean(), o[0, wref.DOF], o[:, wref.NEV].max()))
    for pull in (pp, pd):
        assert abs(pull.mean()) <= 5 / np.sqrt(n)
        assert abs(pull.std() - 1) <= 5 / np.sqrt(2 * n)
    assert (o[:, wref.DOF] == 2 * 127 * 16 - 16 - 2).all()
    assert abs(chi2r.mean() - 1) <= 5 * np.sqrt(2.0 / (o[0, wref.DOF] * n))


def test_model_converges_where_the_narrowband_fit_fails():
    """16 channels of 256 bins at b / b_err = 3 per channel, 200 draws: the
    wideband model converges in every draw and its phase and DM stay within 5
    of their error bars, while the per-channel model (tests/toa_ref.py) leaves
    more than 2 % of its fits beyond 5 sigma -- its coarse maximum picks a
    noise peak."""
    c = wref.low_signal(200, snr=3.0)
    o, _ = wref.wide_ref(*wref.model_args(c))
    pp = ref.circ(o[:, wref.PHI] - c["phi"]) / o[:, wref.PHI_ERR]
    pd = (o[:, wref.D] - c["d"]) / o[:, wref.D_ERR]
    nb = ref.fftfit_ref(c["profiles"].reshape(-1, 256), c["spec"][0], 256).reshape(16, 200, 8)
    pull = ref.circ(nb[:, :, 0] - c["tau"][:, None]) / nb[:, :, 1]
    far = float((np.abs(pull) > 5).mean())
    print("wideband: status 0 in %d of 200, evaluations max %d, pulls std %.3f (phi) %.3f (d), max |pull| %.2f; "
          "narrowband: b / b_err median %.2f, %.1f %% beyond 5 sigma"
          % ((o[:, wref.STATUS] == 0).sum(), o[:, wref.NEV].max(), pp.std(), pd.std(),
             max(np.abs(pp).max(), np.abs(pd).max()), np.median(nb[:, :, 6]), 100 * far))
    assert (o[:, wref.STATUS] == 0).all()
    assert np.abs(pp).max() <= 5 and np.abs(pd).max() <= 5
    assert far > 0.02


def test_model_corners():
    """A zero-weight channel and a NaN channel are left out and reported; one
    usable channel, all weights zero and equal kappa give status 2."""
    c = wref.case_inputs(64, 5, 2, True, 64, 1)
    prof, wt = c["profiles"].copy(), c["wt"].copy()
    prof[1, 0, 7] = np.nan
    wt[3, :] = 0.0
    args = (c["spec"], c["nharm"], c["kappa"], c["phi0"])
    o, p = wref.wide_ref(prof, *args, wt)
    assert list(o[:, wref.NUSED]) == [3, 4] and list(o[:, wref.DOF]) == [2 * 31 * 3 - 5, 2 * 31 * 4 - 6]
    assert not o[:, wref.STATUS].any()
    assert np.isnan(p[1, 0, 0]) and p[3, 0, 0] == 0 and np.isinf(p[[1, 3], 0, 1]).all() and not p[[1, 3], 0, 3].any()
    keep = [0, 2, 4]
    o2, p2 = wref.wide_ref(prof[keep], c["spec"][keep], c["nharm"], c["kappa"][keep], c["phi0"][keep], wt[keep])
    assert np.array_equal(o2[0], o[0]) and np.array_equal(p2[:, 0], p[keep, 0])
    for w in (np.where(np.arange(5)[:, None] == 2, wt, 0), np.zeros_like(wt)):
        o, _ = wref.wide_ref(prof, *args, w.astype(np.float32))
        assert (o[:, wref.STATUS] == 2).all() and np.isinf(o[:, [wref.PHI_ERR, wref.D_ERR]]).all()
        assert not o[:, wref.NEV].any()
    o, _ = wref.wide_ref(prof, c["spec"], c["nharm"], np.full(5, 3.0), c["phi0"], c["wt"])
    assert (o[:, wref.STATUS] == 2).all()


def test_gpu_inputs_converge_and_keep_clear_of_near_tied_peaks():
    """The cases of tests/test_gpu_toa_wide.py under the model alone: status 0
    within 32 evaluations in at least 99 % of the sub-integrations, the two
    highest distinct peaks of the coarse correlation within 1e-3 of each other
    in at most 1 %."""
    total = conv = ties = 0
    worst = 0
    for nbin, per_chan, nharm, ndm, nchan, nsub in wref.all_cases():
        c = wref.case_inputs(nbin, nchan, nsub, per_chan, nharm, ndm)
        o, _, t = wref._fit(*wref.model_args(c), False)
        total += nsub
        conv += int((o[:, wref.STATUS] == 0).sum())
        ties += int(t.sum())
        worst = max(worst, int(o[:, wref.NEV].max()))
    print("%d of %d sub-integrations converged (evaluations: max %d), %d near ties" % (conv, total, worst, ties))
    assert total > 500 and conv >= 0.99 * total and ties <= 0.01 * total


# ---------------------------------------------------------------------------
# the planner and the result class
# ---------------------------------------------------------------------------
def test_plan_keeps_float64_at_hundreds_of_turns():
    """kappa x dm is hundreds of turns at the bottom of the band: phi0 is its
    fraction to 1e-12 turns against exact decimal arithmetic on the float64
    kappa."""
    from psrsigsim_amd.telescope.toa import wideband_plan
    from psrsigsim_amd.utils.constants import DM_K_VALUE
    freqs = np.linspace(1150.0, 1650.0, 33)
    P, dm = 0.0016, 71.0237
    kappa, phi0 = wideband_plan(freqs, P, dm)
    assert kappa.dtype == np.float64 and phi0.dtype == np.float64
    assert np.allclose(kappa, DM_K_VALUE / freqs ** 2 / P, rtol=1e-15) and (kappa * dm).max() > 100
    assert (phi0 >= -0.5).all() and (phi0 < 0.5).all()
    for k, p in zip(kappa, phi0):
        t = Decimal(float(k)) * Decimal(dm)
        f = t - t.to_integral_value()
        d = abs(float(f) - p)
        assert min(d, 1 - d) < 1e-12


def _result(o, p, freqs, P, sublen=10.0, dm=0.0):
    from psrsigsim_amd.telescope import WidebandTOAs
    return WidebandTOAs(o, p, freqs, P, sublen, dm)


def test_ref_freq_decorrelates_phase_and_dm():
    """The phase at ``ref_freq`` against a direct re-fit with the phases
    referred to that frequency (kappa - kappa_0): the same phase and error bar,
    no covariance left."""
    from psrsigsim_amd.telescope.toa import wideband_plan
    from psrsigsim_amd.utils.constants import DM_K_VALUE
    nchan, nbin, P, dm0 = 16, 256, 0.004, 12.5
    freqs = np.linspace(1200.0, 1600.0, nchan)
    kappa, phi0 = wideband_plan(freqs, P, dm0)
    rng = np.random.default_rng(3)
    tm = ref.make_template(nbin)[None]
    spec = ref.template_table(tm, 32)
    phi, d = np.array([0.3, -0.499, 0.01]), np.array([2e-4, -1e-4, 3e-4])
    prof = np.empty((nchan, 3, nbin))
    wt = np.empty((nchan, 3), np.float32)
    for s in range(3):
        prof[:, s], sf2 = wref.portrait(tm, phi0 + phi[s] + kappa * d[s], np.ones(nchan), 30.0, spec, rng)
        wt[:, s] = 1.0 / sf2
    o, p = wref.wide_ref(prof, spec, 32, kappa, phi0, wt)
    t = _result(o, p, freqs, P, dm=dm0)
    assert not t.status.any() and np.allclose(t.dm, dm0 + o[:, wref.D]) and t.dm_nominal == dm0
    k0 = -o[:, wref.COV] / o[:, wref.D_ERR] ** 2
    assert np.allclose(t.ref_freq, np.sqrt(DM_K_VALUE / (P * k0))) and (t.ref_freq > 1200).all() and (t.ref_freq < 1600).all()
    assert (t.shift_ref_err < t.shift_err).all()
    for s in range(3):
        o2, _ = wref.wide_ref(prof[:, s:s + 1], spec, 32, kappa - k0[s], phi0, wt[:, s:s + 1])
        assert abs(ref.circ(o2[0, wref.PHI] - t.shift_ref[s])) < 1e-7
        assert abs(o2[0, wref.PHI_ERR] / t.shift_ref_err[s] - 1) < 1e-6
        assert abs(o2[0, wref.COV]) < 1e-6 * o2[0, wref.PHI_ERR] * o2[0, wref.D_ERR]
        assert abs(o2[0, wref.D] - o[s, wref.D]) < 1e-3 * o[s, wref.D_ERR]
    mid = (np.arange(3) + 0.5) * 10.0
    assert np.allclose(t.t_sec, mid + P * ref.circ(ref.circ(k0 * dm0) + t.shift_ref), rtol=0, atol=1e-12)
    assert np.allclose(t.chi2r, o[:, wref.CHI2] / o[:, wref.DOF]) and t.used.all() and t.scale.shape == (nchan, 3)
    assert t.nev.dtype == np.int32 and t.nchan_used.tolist() == [nchan] * 3


def test_write_tim_carries_the_wideband_flags(tmp_path):
    freqs = np.linspace(1200.0, 1600.0, 4)
    P, sublen = 0.0123456789, 43200.0                          # the third sub-integration crosses midnight
    o = np.zeros((3, 10))
    o[:, 0], o[:, 1], o[:, 2], o[:, 3] = (0.25, -0.5, 0.1), 2e-4, (1e-3, -2e-3, 0.0), 5e-4
    o[:, 4] = -0.8 * 2e-4 * 5e-4
    o[:, 5], o[:, 6], o[:, 7], o[:, 8] = 100.0, 98.0, 4, 5
    o[1, 9] = 1                                                # the iteration cap: not written
    p = np.ones((4, 3, 4))
    t = _result(o, p, freqs, P, sublen, dm=10.0)
    path = str(tmp_path / "w.tim")
    imjd, smjd = 60000, "12345.678901234567"
    assert t.write_tim(path, imjd, smjd, site="gbt", name="J0000+0000") == 2
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] == "FORMAT 1" and len(lines) == 3
    for line, s in zip(lines[1:], (0, 2)):
        name, freq, mjd, e_us, site, f1, dm, f2, dme = line.split()
        assert (name, site, f1, f2) == ("J0000+0000", "gbt", "-pp_dm", "-pp_dme")
        assert abs(float(freq) - t.ref_freq[s]) < 1e-6 and abs(float(e_us) - t.shift_ref_err[s] * P * 1e6) < 1e-6
        assert abs(float(dm) - t.dm[s]) < 1e-10 and abs(float(dme) - 5e-4) < 1e-10
        assert re.fullmatch(r"\d{5}\.\d{16}", mjd)
        want = Decimal(imjd) * 86400 + Decimal(smjd) + Decimal(float(t.t_sec[s]))
        assert abs(Decimal(mjd) * 86400 - want) < Decimal("1e-9")
    assert lines[2].split()[2].startswith("60001.")
    with pytest.raises(ValueError, match="imjd"):
        t.write_tim(path, 60000.5, 0)
    assert abs(t.shift_ref_err[0] - 2e-4 * 0.6) < 1e-12        # sqrt(1 - 0.8^2)


def test_stage_rejections_touch_no_device():
    import torch
    B = _Backend()
    be = B(samprate=0.01)
    t = B.toa_template(ref.make_template(64), 64)
    host = torch.zeros((2, 128))
    k, w = np.ones(2), np.ones((2, 2))
    for args, kw, word in (
            ((host, 2, 2, 32, t, k, k, w), {}, "the template has 64 bins"), ((host, 2, 2, 64, "t", k, k, w), {}, "TOATemplate"),
            ((host, 3, 2, 64, t, k, k, w), {}, "device tensor"), ((host, 2, 0, 64, t, k, k, w), {}, "device tensor"),
            ((host, 2.5, 2, 64, t, k, k, w), {}, "integers"),
            ((host, 2, 2, 64, t, k, k, w), dict(ndm=2), "ndm 2 is not odd"), ((host, 2, 2, 64, t, k, k, w), dict(ndm=0), "ndm 0"),
            ((host, 2, 2, 64, t, k, k, w), dict(ndm=3, dm_step=-1.0), "dm_step"),
            ((host, 2, 2, 64, t, k, k, w), dict(ndm=3, dm_step=np.nan), "dm_step"),
            ((host, 2, 2, 64, t, np.ones(3), k, w), {}, "kappa has the shape"), ((host, 2, 2, 64, t, k, np.ones(1), w), {}, "phi0 has"),
            ((host, 2, 2, 64, t, k, k, np.ones((2, 3))), {}, "wt has the shape")):
        with pytest.raises(ValueError, match="fit_wideband.*" + word):
            be.fit_wideband(*args, **kw)

    class Search(object):
        fold = False

        def __getattr__(self, name):
            raise AssertionError("the signal was touched (%s)" % name)

    with pytest.raises(ValueError, match="fold-mode"):
        be.wideband_toas(Search())

    class Fold(object):
        fold, nsub, Nchan, shard, dm = True, 2, 4, (0, 4), None
        data = torch.zeros((4, 128))

    with pytest.raises(ValueError, match="needs a pulsar or a template"):
        be.wideband_toas(Fold())
    sig = Fold()
    sig.nsub = 3
    with pytest.raises(ValueError, match="3 sub-integrations do not divide a row of 128 samples"):
        be.wideband_toas(sig, template=t)
    sig = Fold()
    sig.shard, sig.data = (1, 3), torch.zeros((2, 128))
    with pytest.raises(ValueError, match="channels 1 .. 3 of 4; a wideband fit needs every channel"):
        be.wideband_toas(sig, template=t)
    with pytest.raises(ValueError, match="ndm 4 is not odd"):
        be.wideband_toas(Fold(), template=t, ndm=4)


# ---------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_hashed():
    from psrsigsim_amd import build
    with open(os.path.join(ROOT, "include", "pss_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+pss_toa_wide_fit\s*\(", header)
    assert re.search(r"\bint64_t\s+pss_toa_wide_workspace_bytes\s*\(", header)
    L = _lib.load()
    assert len(_lib.EXPORTS["pss_toa_wide_fit"][1]) == 20 and hasattr(L, "pss_toa_wide_fit")
    assert len(_lib.EXPORTS["pss_toa_wide_workspace_bytes"][1]) == 5 and hasattr(L, "pss_toa_wide_workspace_bytes")
    assert re.search(r"\bint\s+pss_toa_wide_stages\s*\(", header)
    assert len(_lib.EXPORTS["pss_toa_wide_stages"][1]) == 22 and hasattr(L, "pss_toa_wide_stages")
    assert "pss_toa_wide.hip" in build.UNITS and any(d.endswith("pss_toa_wide.hip") for d in build.DEPS)
    assert any(d.endswith("pss_toa.hpp") for d in build.DEPS)


def test_workspace_bytes():
    L = _lib.load()
    K, nchan, nsub, ndm = 1023, 2048, 15, 3
    n = L.pss_toa_wide_workspace_bytes(nchan, nsub, 2048, 4000, ndm)
    x = nchan * nsub * K * 8
    assert n % 16 == 0 and x < n < x + nchan * nsub * 64 + (1 << 20)
    assert L.pss_toa_wide_workspace_bytes(nchan, nsub, 2048, 4000, 5) > n
    for bad in ((0, 1, 64, 5, 1), (1, 0, 64, 5, 1), (1, 1, 7, 5, 1), (1, 1, 8193, 5, 1), (1, 1, 64, 0, 1), (1, 1, 64, 5, 2),
                (1, 1, 64, 5, 0)):
        assert L.pss_toa_wide_workspace_bytes(*bad) == 0, bad


def test_entry_point_validates_arguments():
    """Every PSS_EINVAL of pss_toa_wide_fit with NULL or host pointers: the
    checks precede any launch (no GPU touched)."""
    p = host_pointer()
    L = _lib.load()
    need = L.pss_toa_wide_workspace_bytes(2, 3, 64, 5, 3)
    good = dict(data=p, nchan=2, nsub=3, nbin=64, ld=192, tspec=p, ntmpl=2, nharm=5, kappa=p, phi0=p, wt=p, ndm=3,
                dm_step=0.5, out=p, out_ld=10, prof=p, prof_ld=4, work=p, work_bytes=need)
    check_rejections(L.pss_toa_wide_fit, good, (
        (dict(data=None), "data is NULL"), (dict(tspec=None), "tspec is NULL"), (dict(out=None), "out is NULL"),
        (dict(kappa=None), "kappa is NULL"), (dict(phi0=None), "phi0 is NULL"), (dict(wt=None), "wt is NULL"),
        (dict(prof=None), "prof is NULL"), (dict(work=None), "work is NULL"),
        (dict(nchan=0), "nchan 0 < 1"), (dict(nchan=-2), "nchan -2 < 1"), (dict(nsub=0), "nsub 0 < 1"),
        (dict(nbin=7, ld=21), "nbin 7 outside [8, 8192]"), (dict(nbin=8193, ld=3 * 8193), "nbin 8193 outside"),
        (dict(ld=191), "ld 191 < nsub 3 x nbin 64"), (dict(out_ld=9), "out_ld 9 < 10"), (dict(prof_ld=3), "prof_ld 3 < 4"),
        (dict(ntmpl=3), "ntmpl 3 is neither 1 nor nchan 2"), (dict(nharm=0), "nharm 0 < 1"),
        (dict(ndm=2), "ndm 2 is not odd"), (dict(ndm=0), "ndm 0 is not odd"), (dict(ndm=-1), "ndm -1"),
        (dict(dm_step=-0.5), "dm_step -0.5 is not finite and >= 0"), (dict(dm_step=float("nan")), "dm_step nan"),
        (dict(dm_step=float("inf")), "dm_step inf"),
        (dict(work_bytes=need - 1), "a workspace of %d bytes, %d needed" % (need - 1, need)),
        (dict(work_bytes=0), "a workspace of 0 bytes"),
    ), prefix="toa_wide_fit: ")
    good.update(first=1, last=2)
    check_rejections(L.pss_toa_wide_stages, good, (
        (dict(first=-1), "stages -1 .. 2 are not within 0 .. 3"), (dict(last=4), "stages 1 .. 4"),
        (dict(first=3), "stages 3 .. 2"), (dict(work=None), "work is NULL"), (dict(ndm=2), "ndm 2 is not odd"),
    ), prefix="toa_wide_stages: ")
