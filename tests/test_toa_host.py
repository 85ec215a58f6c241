"""Host side of the arrival-time stage (no GPU): the float64 model of
``pss_toa_fit`` (tests/toa_ref.py) on noise-free shifts and in a Monte-Carlo of
its error bars, the template planner ``Backend.toa_template``, the C ABI's
argument checks (they precede any launch), ``TOAs.fit_dm`` and ``write_tim``,
and that the inputs of the GPU tests keep clear of near-tied peaks."""
import os
import re
from decimal import Decimal

import numpy as np
import pytest

from psrsigsim_amd import _lib
from tests import toa_ref as ref
from tests.kernel_harness import check_rejections, host_pointer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _Backend():
    from psrsigsim_amd.telescope import Backend
    return Backend


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nbin", (256, 97, 50, 8))
@pytest.mark.parametrize("kind", ("multi", "inter"))
def test_model_returns_the_injected_shift(nbin, kind):
    """Noise-free profiles a + b s(phi - tau0), s rebuilt from the rounded
    table so that the table is exact for them: tau0 to 1e-9 turns (circular),
    b and a to 1e-9 relative, over [-1/2, 1/2) and within 1 / N of +-1/2 and of
    0, where the bracket of the refinement wraps."""
    for nharm in (nbin, max(2, nbin // 8)):
        s, spec = ref.band_limited(ref.make_template(nbin, kind), nharm)
        e = 1.0 / nbin
        tau0 = np.concatenate([np.linspace(-0.5, 0.5, 37, endpoint=False),
                               [-0.5 + 0.3 * e, -0.5 + 0.9 * e, 0.5 - 0.3 * e, 0.5 - 0.9 * e, 0.3 * e, -0.3 * e,
                                0.99 * e, -0.99 * e, 3.5 * e, 0.5 - 1e-7]])
        b0, a0 = 2.5, -0.7
        o = ref.fftfit_ref(ref.shifted(s, tau0, b0, a0), spec, nharm)
        d = np.abs(ref.circ(o[:, 0] - tau0))
        print("nbin %d %s nharm %d: |tau - tau0| max %.3g, b rel %.3g, a rel %.3g"
              % (nbin, kind, nharm, d.max(), np.abs(o[:, 2] / b0 - 1).max(), np.abs(o[:, 4] / a0 - 1).max()))
        assert d.max() <= 1e-9
        assert np.abs(o[:, 2] / b0 - 1).max() <= 1e-9 and np.abs(o[:, 4] / a0 - 1).max() <= 1e-9
        assert (o[:, 0] >= -0.5).all() and (o[:, 0] < 0.5).all() and not o[:, 7].any()


def test_model_error_bars_in_a_monte_carlo():
    """2000 draws of Gaussian noise on a two-component template, N = 256, b /
    b_err about 135: the pulls of tau and of b have |mean| <= 5 / sqrt(n) and a
    standard deviation within 1 +- 5 / sqrt(2 n); rms returns the injected
    noise."""
    n, N, sigma, b0, tau0 = 2000, 256, 0.05, 1.5, 0.1234
    ph = np.arange(N) / N
    tm = np.exp(-0.5 * ((ph - 0.4) / 0.03) ** 2) + 0.5 * np.exp(-0.5 * ((ph - 0.5) / 0.06) ** 2)
    s, spec = ref.band_limited(tm, N)
    rng = np.random.default_rng(20261021)
    prof = ref.shifted(s, tau0, b0, 0.3) + sigma * rng.standard_normal((n, N))
    o = ref.fftfit_ref(prof, spec, N)
    assert not o[:, 7].any() and (o[:, 6] >= 50).all()
    pt = ref.circ(o[:, 0] - tau0) / o[:, 1]
    pb = (o[:, 2] - b0) / o[:, 3]
    print("snr %.1f; tau pull mean %.4f std %.4f; b pull mean %.4f std %.4f; rms %.5f"
          % (np.median(o[:, 6]), pt.mean(), pt.std(), pb.mean(), pb.std(), o[:, 5].mean()))
    for pull in (pt, pb):
        assert abs(pull.mean()) <= 5 / np.sqrt(n)
        assert abs(pull.std() - 1) <= 5 / np.sqrt(2 * n)
    assert abs(o[:, 5].mean() / sigma - 1) < 0.01


def test_model_corners():
    N = 64
    s, spec = ref.band_limited(ref.make_template(N), N)
    good = ref.shifted(s, 0.2, 1.0, 0.0)[0]
    nan = good.copy()
    nan[5] = np.nan
    o = ref.fftfit_ref(np.stack([good, np.full(N, 3.0), np.zeros(N), nan]), spec, N)
    assert list(o[:, 7]) == [0, 2, 2, 2]
    for row, a in ((o[1], 3.0), (o[2], 0.0)):                   # constant: C = 0
        assert row[0] == 0 and np.isinf(row[1]) and row[2] == 0 and np.isinf(row[3]) and row[4] == a
        assert row[5] == 0 and row[6] == 0
    assert o[3, 0] == 0 and np.isinf(o[3, 1]) and np.isinf(o[3, 3]) and np.isnan(o[3, [2, 4, 5, 6]]).all()
    one = ref.fftfit_ref(good, ref.template_table(s, 1), 1)[0]  # K = 1: no degree of freedom
    assert one[7] == 0 and np.isinf(one[[1, 3, 5]]).all() and one[6] == 0 and abs(ref.circ(one[0] - 0.2)) < 1e-6


def test_gpu_inputs_keep_clear_of_near_tied_peaks():
    """The cases of tests/test_gpu_toa.py: the model alone finds its two highest
    local maxima of C within 1e-3 of each other in at most 1 % of them."""
    total = ties = 0
    for nbin in ref.FFT_BINS + ref.DIRECT_BINS:
        for per_chan in (False, True):
            for nharm in ref.nharms(nbin):
                for nchan, nsub in ref.shapes(nbin):
                    prof, spec, _ = ref.case_inputs(nbin, nchan, nsub, per_chan, nharm)
                    t = ref.near_tie(prof.reshape(-1, nbin), ref.per_profile(spec, nsub), nharm)
                    total += t.size
                    ties += int(t.sum())
    print("%d near ties among %d profiles" % (ties, total))
    assert total > 4000 and ties <= 0.01 * total


# ---------------------------------------------------------------------------
# the planner
# ---------------------------------------------------------------------------
def test_template_is_the_rounded_rfft_of_calc_profiles():
    from psrsigsim_amd.pulsar import GaussPortrait, Pulsar
    from psrsigsim_amd.telescope import TOATemplate
    B = _Backend()
    peaks = np.array([0.3, 0.55])
    for nbin, nharm, K in ((256, None, 127), (256, 40, 40), (256, 1000, 127), (97, None, 48), (97, 48, 48), (8, 1, 1)):
        port = GaussPortrait(peak=peaks, width=np.array([0.02, 0.05]), amp=np.array([1.0, 0.4]))
        want = np.fft.rfft(np.asarray(port.calc_profiles(np.arange(nbin) / nbin, Nchan=4), dtype=np.float64)[:1],
                           axis=1)[:, :K + 1]
        for source in (port, Pulsar(0.005, 1.0, profiles=port)):
            t = B.toa_template(source, nbin, Nchan=4, nharm=nharm)
            assert isinstance(t, TOATemplate) and (t.nbin, t.K, t.ntmpl) == (nbin, K, 1)      # rows alike: one
            assert t.spec.dtype == np.float32 and t.spec.shape == (1, K + 1, 2)
            assert np.array_equal(t.spec[..., 0], want.real.astype(np.float32))
            assert np.array_equal(t.spec[..., 1], want.imag.astype(np.float32))
            s = t.spec.astype(np.float64)
            assert abs(t.S2[0] / (s[0, 1:] ** 2).sum() - 1) < 1e-14 and t.S0[0] == s[0, 0, 0]
    rows = np.stack([ref.make_template(50), 2 * ref.make_template(50, "inter")])
    t = B.toa_template(rows, 50)
    assert (t.ntmpl, t.K) == (2, 24) and np.array_equal(t.spec, ref.template_table(rows, 50))
    assert B.toa_template(rows[0], 50, nharm=3).spec.shape == (1, 4, 2)


def test_template_rejections():
    B = _Backend()
    tm = ref.make_template(64)
    for args, kw, word in (((tm, 63), {}, "shape"), ((tm, 4), {}, "nbin 4 outside"), ((tm, 16384), {}, "outside"),
                           ((tm, 64), dict(nharm=0), "nharm 0 < 1"), ((tm, 64.5), {}, "integers"),
                           ((np.ones(64), 64), {}, "template row 0 has no power"),
                           ((np.stack([tm, np.full(64, 2.0)]), 64), {}, "template row 1 has no power"),
                           ((np.stack([tm, tm * 2, tm * 3]), 64), dict(Nchan=2), "3 template rows for 2 channels"),
                           ((np.where(np.arange(64) == 3, np.nan, tm), 64), {}, "not finite")):
        with pytest.raises(ValueError, match="toa_template: .*" + re.escape(word)):
            B.toa_template(*args, **kw)
    # a cosine at harmonic 2 has no power in harmonic 1
    with pytest.raises(ValueError, match="no power in the harmonics 1 .. 1"):
        B.toa_template(np.round(np.cos(4 * np.pi * np.arange(8) / 8)), 8, nharm=1)


def test_stage_rejections_touch_no_device():
    import torch
    B = _Backend()
    be = B(samprate=0.01)
    t = B.toa_template(ref.make_template(64), 64)
    host = torch.zeros((2, 128))
    for args, word in (((host, 2, 2, 32, t), "the template has 64 bins"), ((host, 2, 2, 64, "t"), "TOATemplate"),
                       ((host, 3, 2, 64, t), "device tensor"), ((host, 2, 3, 64, t), "device tensor"),
                       ((host, 2, 0, 64, t), "device tensor"), ((host, 2.5, 2, 64, t), "integers"),
                       ((host, 2, 2, 64, B.toa_template(np.stack([ref.make_template(64)] * 3)
                                                        * np.arange(1, 4)[:, None], 64)), "3 templates for 2")):
        with pytest.raises(ValueError, match=word):
            be.fit_profiles(*args)

    class Search(object):
        fold = False

        def __getattr__(self, name):
            raise AssertionError("the signal was touched (%s)" % name)

    with pytest.raises(ValueError, match="fold-mode"):
        be.toas(Search())


# ---------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_hashed():
    from psrsigsim_amd import build
    with open(os.path.join(ROOT, "include", "pss_hip.h")) as f:
        header = f.read()
    assert re.search(r"\bint\s+pss_toa_fit\s*\(", header)
    assert len(_lib.EXPORTS["pss_toa_fit"][1]) == 11 and hasattr(_lib.load(), "pss_toa_fit")
    assert "pss_toa.hip" in build.UNITS and any(d.endswith("pss_toa.hip") for d in build.DEPS)


def test_entry_point_validates_arguments():
    """Every PSS_EINVAL of pss_toa_fit with NULL or host pointers: the checks
    precede any launch (no GPU touched)."""
    p = host_pointer()
    big = (1 << 31) - 1
    good = dict(data=p, nchan=2, nsub=3, nbin=64, ld=192, tspec=p, ntmpl=2, nharm=5, out=p, out_ld=8)
    check_rejections(_lib.load().pss_toa_fit, good, (
        (dict(data=None), "data is NULL"), (dict(tspec=None), "tspec is NULL"), (dict(out=None), "out is NULL"),
        (dict(nchan=0), "nchan 0 < 1"), (dict(nchan=-2), "nchan -2 < 1"), (dict(nsub=0), "nsub 0 < 1"),
        (dict(nbin=7, ld=21), "nbin 7 outside [8, 8192]"), (dict(nbin=8193, ld=3 * 8193), "nbin 8193 outside"),
        (dict(nbin=0), "nbin 0 outside"), (dict(ld=191), "ld 191 < nsub 3 x nbin 64"), (dict(out_ld=7), "out_ld 7 < 8"),
        (dict(ntmpl=3), "ntmpl 3 is neither 1 nor nchan 2"), (dict(ntmpl=0), "ntmpl 0"), (dict(nharm=0), "nharm 0 < 1"),
        # the grid: a workgroup a profile (direct path), 128 profiles a workgroup at 64 bins
        (dict(nchan=big, ntmpl=1, nsub=2, nbin=50, ld=100), "4294967294 workgroups exceed 2^31 - 1"),
        (dict(nchan=big, ntmpl=1, nsub=big, ld=big * 64), "36028796985409537 workgroups exceed 2^31 - 1"),
    ), prefix="toa_fit: ")


# ---------------------------------------------------------------------------
# TOAs
# ---------------------------------------------------------------------------
def _toas(shift, err, freqs, period=0.004, sublen=10.0, status=None):
    from psrsigsim_amd.telescope import TOAs
    fit = np.zeros(shift.shape + (8,))
    fit[..., 0], fit[..., 1] = shift, err
    fit[..., 2], fit[..., 3], fit[..., 6] = 1.0, 0.01, 100.0
    if status is not None:
        fit[..., 7] = status
    return TOAs(fit, freqs, period, sublen)


def test_fit_dm_recovers_an_injected_dm_within_its_error():
    from psrsigsim_amd.utils.constants import DM_K_VALUE
    rng = np.random.default_rng(5)
    freqs = np.linspace(1200.0, 1600.0, 16)
    P, dm0 = 0.004, 0.35                                       # 0.35 pc/cm^3: 1 ms .. 0.57 ms across the band
    err = np.broadcast_to(rng.uniform(1e-4, 5e-4, (16, 1)), (16, 6)).copy()
    pulls = []
    for trial in range(40):
        shift = (DM_K_VALUE * dm0 / freqs ** 2)[:, None] / P + 0.013 + err * rng.standard_normal((16, 6))
        status = np.zeros((16, 6))
        shift[3, 2], status[3, 2] = 0.4, 2                     # a degenerate fit does not enter
        t = _toas(ref.circ(shift), err, freqs, P, status=status)
        dm, dm_err, chi2r = t.fit_dm()
        dm2, dm_err2, _ = t.fit_dm(ref_freq=1400.0)
        assert abs(dm - dm2) < 1e-9 and abs(dm_err - dm_err2) < 1e-12
        assert abs(dm - dm0) < 5 * dm_err and 0.5 < chi2r < 1.6
        pulls.append((dm - dm0) / dm_err)
    print("fit_dm pulls: mean %.3f std %.3f" % (np.mean(pulls), np.std(pulls)))
    assert abs(np.mean(pulls)) < 5 / np.sqrt(40) and abs(np.std(pulls) - 1) < 5 / np.sqrt(80)
    assert np.allclose(t.delay_ms(), t.shift * P * 1e3) and t.status.dtype == np.int32
    assert np.allclose(t.t_sec, (np.arange(6) + 0.5)[None, :] * 10.0 + t.shift * P)
    with pytest.raises(ValueError, match="fit_dm"):
        _toas(np.zeros((1, 5)), np.ones((1, 5)), np.array([1400.0])).fit_dm()


def test_write_tim_round_trips_the_mjd_below_a_nanosecond(tmp_path):
    freqs = np.array([1400.0, 1500.25])
    shift = np.array([[0.25, -0.125, 0.0], [0.4999, -0.5, 0.1]])
    err = np.full((2, 3), 2e-4)
    status = np.zeros((2, 3))
    status[1, 1] = 1                                           # the iteration cap: not written
    P, sublen = 0.0123456789, 43200.0                          # the third sub-integration crosses midnight
    t = _toas(shift, err, freqs, P, sublen, status)
    path = str(tmp_path / "x.tim")
    imjd, smjd = 60000, "12345.678901234567"
    assert t.write_tim(path, imjd, smjd, site="gbt", name="J0000+0000") == 5
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] == "FORMAT 1" and len(lines) == 6
    cells = [(c, s) for c in range(2) for s in range(3) if not (c == 1 and s == 1)]
    for line, (c, s) in zip(lines[1:], cells):
        name, freq, mjd, e_us, site = line.split()
        assert (name, site) == ("J0000+0000", "gbt") and float(freq) == freqs[c]
        assert abs(float(e_us) - 2e-4 * P * 1e6) < 1e-6
        assert re.fullmatch(r"\d{5}\.\d{16}", mjd)
        want = Decimal(imjd) * 86400 + Decimal(smjd) + Decimal(float(t.t_sec[c, s]))
        assert abs(Decimal(mjd) * 86400 - want) < Decimal("1e-9")
    assert lines[3].split()[2].startswith("60001.")
    assert t.write_tim(path, 60000, 0.5) == 5                  # seconds as a float
    with pytest.raises(ValueError, match="imjd"):
        t.write_tim(path, 60000.5, 0)
