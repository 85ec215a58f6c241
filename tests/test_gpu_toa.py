"""The template match on the GPU (``pss_toa_fit``, ``Backend.fit_profiles`` /
``toas``) against the float64 model of tests/toa_ref.py.

Tolerance.  The kernel works in float32, the model in float64, so the bound is
what float32 arithmetic itself costs: ``fftfit_f32`` restates the model with
SciPy's single-precision transform, and a GPU value may be 4 x as far from the
model as the restatement's worst value is -- worst over the profiles of the same
configuration (nbin, templates, nharm) and noise level, all shapes together,
computed at run time.  For tau the distance is circular, in turns, with a floor
of 2^-24 (the rounding of a float32 in [-1/2, 1/2)); for b, a, rms and the two
errors it is relative to the fitted signal (``_scale``) with the same floor;
snr must be the float32 quotient of the b and b_err next to it.  Where the model
gives an infinity or a NaN the kernel must give exactly that.  tau must also stay within a tenth
of the model's error bar, max(0.1 tau_err, 2^-24): on a noise-free profile the
model's error bar measures the rounding of the float32 samples alone (1e-9
turns and less), below what a float32 tau can resolve at all, so the floor of
the output's own rounding holds there as well.  ``status`` is equal.  A profile
whose two highest local maxima of the model's coarse correlation lie within
1e-3 of each other is left out (tests/test_toa_host.py asserts that these are
at most 1 % of the cases, from the model alone).

Measured on an MI355X, worst over all cases, as a fraction of its bound: see
the figures every test prints and DESIGN.md section 9.

Every case gives the kernel views inside larger tensors (kernel_harness): the
rows of data with a stride ld > nsub nbin between guards of 2^20, out with a row
stride of 11 inside a sentinel that is checked untouched.
"""
import numpy as np
import pytest

from tests import toa_ref as ref
from tests import kernel_harness as kh
from tests.kernel_harness import engine_seed_restored, same_bits  # noqa: F401 (the fixture is autouse here)

pytestmark = pytest.mark.gpu

IN_GUARD = float(1 << 20)
OUT_GUARD = -7.0
FLOOR = 2.0 ** -24
TAU, TAU_ERR, B, B_ERR, A, RMS, SNR, STATUS = range(8)


def run_fit(hip_lib, prof, spec, nharm, ld=None, out_ld=11, in_off=0, out_off=0):
    """pss_toa_fit on profiles [nchan, nsub, nbin]; float32 [nchan * nsub, 8]
    after the guard checks."""
    import torch
    from psrsigsim_amd import _lib
    nchan, nsub, nbin = prof.shape
    ld = (nsub * nbin + 7) // 4 * 4 if ld is None else ld
    data = kh.GuardedInput(prof.reshape(nchan, nsub * nbin), ld, in_off, IN_GUARD)
    out = kh.GuardedOutput(nchan * nsub, 8, out_ld, out_off, OUT_GUARD)
    spec_d = torch.from_numpy(np.ascontiguousarray(spec)).cuda()
    torch.cuda.synchronize()
    rc = hip_lib.pss_toa_fit(data.ptr, nchan, nsub, nbin, ld, spec_d.data_ptr(), spec.shape[0], nharm, out.ptr, out_ld,
                             None)
    _lib.check(rc, "toa_fit")
    torch.cuda.synchronize()
    return out.read()


def _scale(col, want, spec_rows, nbin):
    """The size a column's distance is relative to.  b, b_err: |b|.  a: the
    larger of the two terms it is the difference of.  rms: the rms amplitude
    |b| sqrt(2 S2) / N of the fitted harmonics.  tau_err: the turn
    1 / (2 pi k_rms), k_rms^2 = sum k^2 |S_k|^2 / S2, at which tau_err is
    b_err / b.  The three noise figures are thus compared as noise-to-signal
    ratios: on a noise-free profile they are a rounding residue, 1e-9 in the
    model and 1e-4 in any float32 evaluation, and no bound relative to their
    own value could hold."""
    s = spec_rows.astype(np.float64)
    p2 = s[:, 1:, 0] ** 2 + s[:, 1:, 1] ** 2
    S2 = p2.sum(axis=1)
    k = np.arange(1, s.shape[1], dtype=np.float64)
    b = np.abs(want[:, B])
    if col == A:
        return np.maximum(np.abs(want[:, A]), b * np.abs(s[:, 0, 0]) / nbin)
    if col == RMS:
        return b * np.sqrt(2 * S2) / nbin
    if col == TAU_ERR:
        return np.sqrt(S2 / (p2 * k * k).sum(axis=1)) / (2 * np.pi)
    return b


def _distances(col, got, want, f32, sq_want, sq_f32, spec_rows, nbin):
    """(the kernel's distance to the model, the restatement's, the floor) of a
    column, per profile: turns for tau, relative to ``_scale`` for b and a.
    The three noise figures are compared as squares, linear in the residual R,
    the model's and the restatement's taken before R is clamped at 0
    (``noise_squares``): a restatement whose R comes out below 0 would else
    seem exact.  nan where the model's value is not finite: compared exactly."""
    if col == TAU:
        return (np.abs(ref.circ(got[:, col] - want[:, col])), np.abs(ref.circ(f32[:, col] - want[:, col])),
                np.full(len(got), FLOOR))
    sc = _scale(col, want, spec_rows, nbin)
    with np.errstate(all="ignore"):
        if col in (TAU_ERR, B_ERR, RMS):
            w = sq_want[:, (TAU_ERR, B_ERR, RMS).index(col)]
            f = sq_f32[:, (TAU_ERR, B_ERR, RMS).index(col)]
            dg, df, floor = np.abs(got[:, col] ** 2 - w) / sc ** 2, np.abs(f - w) / sc ** 2, 2 * FLOOR * np.abs(w) / sc ** 2
        else:
            dg, df = np.abs(got[:, col] - want[:, col]) / sc, np.abs(f32[:, col] - want[:, col]) / sc
            floor = np.full(len(got), FLOOR)
    fin = np.isfinite(want[:, col])
    return np.where(fin, dg, np.nan), np.where(fin, df, np.nan), floor


@pytest.mark.parametrize("per_chan", (False, True), ids=("one_template", "template_per_channel"))
@pytest.mark.parametrize("nbin", ref.FFT_BINS + ref.DIRECT_BINS)
def test_agrees_with_the_model(nbin, per_chan, hip_lib):
    worst, fails = np.zeros(8), []
    for nharm in ref.nharms(nbin):
        runs = []
        for nchan, nsub in ref.shapes(nbin):
            prof, spec, _ = ref.case_inputs(nbin, nchan, nsub, per_chan, nharm)
            assert spec.shape[0] == (nchan if per_chan else 1)
            rows = ref.per_profile(spec, nsub)
            p2 = prof.reshape(-1, nbin)
            want, f32 = ref.fftfit_ref(p2, rows, nharm), ref.fftfit_f32(p2, rows, nharm)
            keep = ~ref.near_tie(p2, rows, nharm)
            got = run_fit(hip_lib, prof, spec, nharm).astype(np.float64)
            srow = np.broadcast_to(rows, (len(p2),) + rows.shape[-2:])
            runs.append((got, want, f32, keep, np.arange(len(p2)) % len(ref.SNRS), srow,
                         ref.noise_squares(p2, rows, nharm), ref.noise_squares(p2, rows, nharm, np.float32)))
        got, want, f32, keep, level, srow, sqw, sqf = (np.concatenate([r[i] for r in runs]) for i in range(8))
        assert keep.sum() >= 0.9 * keep.size
        assert np.array_equal(got[keep, STATUS], want[keep, STATUS])
        # snr is b / b_err, one float32 division
        g32 = got.astype(np.float32)
        with np.errstate(all="ignore"):
            q = g32[:, B] / g32[:, B_ERR]
        assert np.array_equal(q[~np.isnan(q)], g32[~np.isnan(q), SNR])
        for col in range(SNR):
            dg, df, floor = _distances(col, got, want, f32, sqw, sqf, srow, nbin)
            exact = np.isnan(dg) & keep
            w, g = want[exact, col], got[exact, col]
            assert np.array_equal(np.isnan(w), np.isnan(g)) and np.array_equal(w[~np.isnan(w)], g[~np.isnan(w)]), \
                (nharm, ref.COLS[col], w, g)
            for lv in range(len(ref.SNRS)):
                m = keep & (level == lv) & ~np.isnan(dg)
                if not m.any():
                    continue
                bound = np.maximum(4 * np.nanmax(df[m]), floor[m])
                if col == TAU:
                    te = want[m, TAU_ERR]
                    ok = np.isfinite(te) & (te != 0)
                    bound = np.where(ok, np.minimum(bound, np.maximum(0.1 * te, FLOOR)), bound)
                ratio = float((dg[m] / bound).max())
                worst[col] = max(worst[col], ratio)
                print("nbin %d nharm %d snr %s %s: gpu %.3g, float32 restatement %.3g, bound %.3g"
                      % (nbin, nharm, ref.SNRS[lv], ref.COLS[col], dg[m].max(), np.nanmax(df[m]), bound.min()))
                if ratio > 1.0:
                    fails.append((nharm, ref.SNRS[lv], ref.COLS[col], round(ratio, 2)))
    print("nbin %d: worst distance / bound per column %s" % (nbin, np.round(worst[:SNR], 3)))
    assert not fails, fails


@pytest.mark.parametrize("nbin", (256, 2048, 1000, 97))
def test_same_bits_in_every_layout_and_run(nbin, hip_lib):
    nchan, nsub, nharm = 3, 5, ref.nharms(nbin)[1]
    prof, spec, _ = ref.case_inputs(nbin, nchan, nsub, True, nharm)
    ld = (nsub * nbin + 7) // 4 * 4
    base = run_fit(hip_lib, prof, spec, nharm, ld=ld, out_ld=12)
    assert same_bits(base, run_fit(hip_lib, prof, spec, nharm, ld=ld, out_ld=12))
    for lay in kh.misaligned_layouts(ld, 12, kh.odd(ld), 11):
        assert same_bits(base, run_fit(hip_lib, prof, spec, nharm, **lay)), lay
    assert same_bits(base, run_fit(hip_lib, prof, spec, nharm, ld=nsub * nbin, out_ld=8))     # no padding at all


@pytest.mark.parametrize("nbin", (64, 2048, 50))
def test_a_profile_does_not_depend_on_its_neighbours(nbin, hip_lib):
    """Every profile of a batch fitted alone (one channel, one sub-integration,
    its own channel's template) gives the bits it has inside the batch."""
    nchan, nsub, nharm = 3, 5, nbin
    prof, spec, _ = ref.case_inputs(nbin, nchan, nsub, True, nharm)
    batch = run_fit(hip_lib, prof, spec, nharm)
    for c in range(nchan):
        for s in range(nsub):
            alone = run_fit(hip_lib, prof[c:c + 1, s:s + 1], spec[c:c + 1], nharm)
            assert same_bits(alone[0], batch[c * nsub + s]), (c, s)


@pytest.mark.parametrize("nbin", (64, 2048, 97))
def test_degenerate_profiles(nbin, hip_lib):
    """A constant profile, an all-zero one and one with a NaN, between ordinary
    profiles: status and outputs as the model says, and the ordinary profiles
    keep the bits they have when ordinary profiles stand in those places."""
    nharm = nbin
    prof, spec, _ = ref.case_inputs(nbin, 1, 7, False, nharm)
    plain = run_fit(hip_lib, prof, spec, nharm)
    bad = prof.copy()
    bad[0, 1] = 3.0
    bad[0, 3] = 0.0
    bad[0, 4, nbin // 3] = np.nan
    bad[0, 6, 0] = np.inf
    got = run_fit(hip_lib, bad, spec, nharm)
    want = ref.fftfit_ref(bad[0], spec[0], nharm)
    for i in (0, 2, 5):
        assert same_bits(got[i], plain[i]), i
    assert list(got[:, STATUS]) == list(want[:, STATUS]) == [0, 2, 0, 2, 2, 0, 2]
    for i in (1, 3):
        assert np.array_equal(got[i].astype(np.float64), want[i]), (i, got[i], want[i])
    for i in (4, 6):
        assert np.array_equal(np.isnan(got[i]), np.isnan(want[i]))
        assert np.array_equal(got[i][~np.isnan(got[i])].astype(np.float64), want[i][~np.isnan(want[i])])


def test_backend_fit_profiles_is_the_entry_point(hip_lib):
    import torch
    from psrsigsim_amd.telescope import Backend
    nbin, nchan, nsub = 256, 3, 5
    prof, spec, _ = ref.case_inputs(nbin, nchan, nsub, True, 40)
    tm = np.stack([ref.make_template(nbin, ("multi", "inter")[c % 2]) * (1 + c / 4) for c in range(nchan)])
    t = Backend.toa_template(tm, nbin, nharm=40)
    assert np.array_equal(t.spec, spec)
    data = torch.from_numpy(prof.reshape(nchan, nsub * nbin)).cuda()
    out = Backend(samprate=0.01).fit_profiles(data, nchan, nsub, nbin, t)
    assert tuple(out.shape) == (nchan, nsub, 8) and out.dtype == torch.float32
    assert same_bits(out.cpu().numpy().reshape(-1, 8), run_fit(hip_lib, prof, spec, 40))


def _fold_signal(seed, dm, fold=True):
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar, GaussProfile
    from psrsigsim_amd.ism import ISM
    from psrsigsim_amd.telescope import Backend, Receiver, telescope as T
    P, nfold = 0.004, 10000                                    # 256 bins at 64 kHz
    pss.seed(seed)
    sig = FilterBankSignal(1400, 400, Nsubband=8, sample_rate=0.064, sublen=P * nfold if fold else None, fold=fold)
    psr = Pulsar(P, 2e-4, profiles=GaussProfile(0.5, 0.05, 1))
    psr.make_pulses(sig, tobs=4 * P * nfold if fold else 0.256)
    ISM().disperse(sig, dm)
    tel = T.Arecibo()
    # equal rates: the backend's 1 / (2 samprate) is the signal's sublen / nbin
    tel.add_system(name="S", receiver=Receiver(fcent=1400, bandwidth=400, name="L"),
                   backend=Backend(samprate=0.064 / (2 * nfold), name="B"))
    assert T.Telescope.resample_branch(sig, tel.systems["S"][1])[0] == "copy" or not fold
    tel.observe(sig, psr, system="S", noise=True)
    return sig, psr, P


def test_toas_close_the_loop_on_an_injected_dm(hip_lib):
    """8 channels x 4 sub-integrations of 256 bins, Nfold = 10^4, DM 0.3 (0.86
    ms .. 0.52 ms of a 4 ms period across the band), radiometer noise at 5.6 x
    the peak of the profile's own chi^2 scatter: the shifts are signal.delay /
    P within 5 shift_err for at least 95 % of the entries, fit_dm returns the
    DM within 5 dm_err.  (The CPU oracle's signal under the float64 model:
    b / b_err 55, largest pull 2.8, DM pulls 0.7, 0.1 and -0.4 at three seeds.)"""
    from psrsigsim_amd._units import to_value
    from psrsigsim_amd.telescope import Backend, TOAs
    dm0 = 0.3
    sig, psr, P = _fold_signal(11, dm0)
    t = Backend(samprate=0.064).toas(sig, psr)
    assert isinstance(t, TOAs) and t.shift.shape == (8, 4) and t.period == P and t.sublen == 40.0
    want = np.asarray(to_value(sig.delay, 'ms'), dtype=np.float64) * 1e-3 / P
    pull = ref.circ(t.shift - want[:, None]) / t.shift_err
    dm, dm_err, chi2r = t.fit_dm()
    print("snr %.1f; pulls: max %.2f std %.2f; dm %.5f +- %.5f (pull %.2f), chi2r %.2f"
          % (np.median(t.snr), np.abs(pull).max(), pull.std(), dm, dm_err, (dm - dm0) / dm_err, chi2r))
    assert not t.status.any() and (t.snr > 20).all()
    assert (np.abs(pull) <= 5).mean() >= 0.95
    assert abs(dm - dm0) <= 5 * dm_err and dm_err < 0.01
    assert np.allclose(t.delay_ms(), t.shift * P * 1e3)
    # the model on the same device data
    nbin = 256
    tm = Backend.toa_template(psr, nbin, Nchan=8)
    model = ref.fftfit_ref(sig.data.cpu().numpy().reshape(32, nbin), tm.spec[0], nbin)
    assert np.abs(ref.circ(model[:, TAU] - t.shift.ravel())).max() <= 0.1 * model[:, TAU_ERR].min()


def test_toas_rejections(hip_lib):
    from psrsigsim_amd.telescope import Backend
    be = Backend(samprate=0.064)
    sig, psr, _ = _fold_signal(3, 0.1, fold=False)
    with pytest.raises(ValueError, match="fold-mode"):
        be.toas(sig, psr)
    sig, psr, _ = _fold_signal(3, 0.1)
    with pytest.raises(ValueError, match="needs a pulsar or a template"):
        be.toas(sig)
    sig._nsub = 3
    with pytest.raises(ValueError, match="3 sub-integrations do not divide a row of 1024 samples"):
        be.toas(sig, psr)
