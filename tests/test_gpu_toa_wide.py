"""The wideband fit on the GPU (``pss_toa_wide_fit``, ``Backend.fit_wideband`` /
``wideband_toas``) against the float64 model of tests/toa_wide_ref.py.

Tolerance: the scheme of tests/test_gpu_toa.py.  ``wide_f32`` restates the
model with single-precision spectra and harmonic sums, and a GPU value may be
4 x as far from the model as the restatement's worst value is -- worst over the
sub-integrations of the same configuration (nbin, templates, nharm, ndm) and
noise level, all shapes together, computed at run time.  For phi the distance
is circular, in turns; for d it is multiplied by kappa's span (max - min), the
turns by which it moves the band's edges against each other; the floor of both
is 2^-24, and neither may lie beyond a tenth of the model's error bar (same
floor).  The error bars, the covariance (relative to phi_err d_err), chi2
(relative to sum wt PP, the chi2 of no fit at all) and b, b_err (relative to
|b|) follow the same scheme with a floor of 2^-20: a term of the sums behind
them has gone through up to sixteen float32 roundings of 2^-24 each (eleven
butterfly stages at 2048 bins, the cross-spectrum, the turn, the products).
``status``, the channels used and dof are equal; the evaluations are printed.
A sub-integration whose two highest distinct coarse peaks lie within 1e-3 of
each other is left out (tests/test_toa_wide_host.py asserts that these are at
most 1 % and that the model converges on at least 99 %).

Every case gives the kernel views inside larger tensors (kernel_harness): the
rows of data with a stride ld > nsub nbin between guards of 2^20, both outputs
with padded rows inside sentinels that are checked untouched, and a workspace
of exactly the advertised size between guard bytes.
"""
import numpy as np
import pytest

from tests import toa_ref as ref
from tests import toa_wide_ref as wref
from tests import kernel_harness as kh
from tests.kernel_harness import engine_seed_restored  # noqa: F401 (the fixture is autouse here)

pytestmark = pytest.mark.gpu

IN_GUARD = float(1 << 20)
OUT_GUARD = -7.0
FLOOR = 2.0 ** -24
FLOOR_SUMS = 2.0 ** -20
WORK_PAD = 4096


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_wide(hip_lib, c, ld=None, in_off=0, out_ld=11, out_off=0, prof_ld=5, prof_off=0, work_off=0):
    """pss_toa_wide_fit on the case ``c``; (float64 [nsub, 10], float32 [nchan,
    nsub, 4]) after the guard checks."""
    import torch
    from psrsigsim_amd import _lib
    prof = c["profiles"]
    nchan, nsub, nbin = prof.shape
    ld = (nsub * nbin + 7) // 4 * 4 if ld is None else ld
    data = kh.GuardedInput(prof.reshape(nchan, nsub * nbin), ld, in_off, IN_GUARD)
    wt = kh.GuardedInput(c["wt"], nsub, 0, IN_GUARD)
    out = kh.GuardedOutput(nsub, 10, out_ld, out_off, OUT_GUARD, dtype=np.float64)
    rows = kh.GuardedOutput(nchan * nsub, 4, prof_ld, prof_off, OUT_GUARD)
    spec = c["spec"]
    spec_d = torch.from_numpy(np.ascontiguousarray(spec)).cuda()
    kap = torch.from_numpy(np.ascontiguousarray(c["kappa"], dtype=np.float64)).cuda()
    ph0 = torch.from_numpy(np.ascontiguousarray(c["phi0"], dtype=np.float64)).cuda()
    need = int(hip_lib.pss_toa_wide_workspace_bytes(nchan, nsub, nbin, c["nharm"], c["ndm"]))
    assert need > 0 and need % 16 == 0
    work = torch.full((need + 2 * WORK_PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    wptr = work.data_ptr() + WORK_PAD + 16 * work_off
    assert wptr % 16 == 0
    torch.cuda.synchronize()
    rc = hip_lib.pss_toa_wide_fit(data.ptr, nchan, nsub, nbin, ld, spec_d.data_ptr(), spec.shape[0], c["nharm"],
                                  kap.data_ptr(), ph0.data_ptr(), wt.ptr, c["ndm"], float(c["dm_step"]), out.ptr,
                                  out_ld, rows.ptr, prof_ld, wptr, need, None)
    _lib.check(rc, "toa_wide_fit")
    torch.cuda.synchronize()
    w = work.cpu().numpy()
    lo = WORK_PAD + 16 * work_off
    assert (w[:lo] == 0xA5).all() and (w[lo + need:] == 0xA5).all(), "written outside the workspace"
    return out.read(), rows.read().reshape(nchan, nsub, 4)


def _columns(o, p, want_o, want_p, span):
    """Per sub-integration, the distances of ``o`` / ``p`` to the model, a dict by column name."""
    with np.errstate(all="ignore"):
        b = np.abs(want_p[:, :, 0])
        none = want_o[:, wref.CHI2] + np.nansum((want_p[:, :, 0] / want_p[:, :, 1]) ** 2, axis=0)
        pe, de = want_o[:, wref.PHI_ERR], want_o[:, wref.D_ERR]
        used = want_p[:, :, 3] != 0
        return {
            "phi": np.abs(ref.circ(o[:, wref.PHI] - want_o[:, wref.PHI])),
            "d x span": np.abs(o[:, wref.D] - want_o[:, wref.D]) * span,
            "phi_err": np.abs(o[:, wref.PHI_ERR] / pe - 1),
            "d_err": np.abs(o[:, wref.D_ERR] / de - 1),
            "cov": np.abs(o[:, wref.COV] - want_o[:, wref.COV]) / (pe * de),
            "chi2": np.abs(o[:, wref.CHI2] - want_o[:, wref.CHI2]) / none,
            "b": np.where(used, np.abs(p[:, :, 0] - want_p[:, :, 0]) / b, 0).max(axis=0),
            "b_err": np.where(used, np.abs(p[:, :, 1] / want_p[:, :, 1] - 1), 0).max(axis=0),
        }


@pytest.mark.parametrize("per_chan", (False, True), ids=("one_template", "template_per_channel"))
@pytest.mark.parametrize("nbin", wref.BINS)
def test_agrees_with_the_model(nbin, per_chan, hip_lib):
    names = ("phi", "d x span", "phi_err", "d_err", "cov", "chi2", "b", "b_err")
    worst, fails, nev_max = dict.fromkeys(names, 0.0), [], 0
    for nharm in wref.nharms(nbin):
        for ndm in wref.NDMS:
            runs = []
            for nchan, nsub in wref.shapes(nbin, nharm):
                c = wref.case_inputs(nbin, nchan, nsub, per_chan, nharm, ndm)
                assert c["spec"].shape[0] == (nchan if per_chan else 1)
                args = wref.model_args(c)
                (wo, wp), (fo, fp) = wref.wide_ref(*args), wref.wide_f32(*args)
                keep = ~wref.near_tie(*args)
                go, gp = run_wide(hip_lib, c)
                gp = gp.astype(np.float64)
                span = c["kappa"].max() - c["kappa"].min()
                assert np.array_equal(go[keep][:, [wref.STATUS, wref.NUSED, wref.DOF]],
                                      wo[keep][:, [wref.STATUS, wref.NUSED, wref.DOF]])
                assert np.array_equal(gp[:, :, 3], wp[:, :, 3])
                assert (go[:, wref.PHI] >= -0.5).all() and (go[:, wref.PHI] < 0.5).all()
                nev_max = max(nev_max, int(go[:, wref.NEV].max()))
                print("nbin %d nharm %d ndm %d %d x %d: evaluations gpu %s model %s"
                      % (nbin, nharm, ndm, nchan, nsub, go[:, wref.NEV].astype(int), wo[:, wref.NEV].astype(int)))
                runs.append((_columns(go, gp, wo, wp, span), _columns(fo, fp, wo, wp, span), keep,
                             np.arange(nsub) % len(wref.SNRS), wo[:, wref.PHI_ERR], wo[:, wref.D_ERR] * span))
            keep, level, pe, de = (np.concatenate([r[i] for r in runs]) for i in (2, 3, 4, 5))
            assert keep.sum() >= 0.9 * keep.size
            for name in names:
                dg = np.concatenate([r[0][name] for r in runs])
                df = np.concatenate([r[1][name] for r in runs])
                for lv in range(len(wref.SNRS)):
                    m = keep & (level == lv)
                    if not m.any():
                        continue
                    floor = FLOOR if name in ("phi", "d x span") else FLOOR_SUMS
                    bound = np.full(m.sum(), max(4 * df[m].max(), floor))
                    if name in ("phi", "d x span"):
                        bound = np.minimum(bound, np.maximum(0.1 * (pe if name == "phi" else de)[m], FLOOR))
                    ratio = float((dg[m] / bound).max())
                    worst[name] = max(worst[name], ratio)
                    print("nbin %d nharm %d ndm %d snr %s %s: gpu %.3g, float32 restatement %.3g, bound %.3g"
                          % (nbin, nharm, ndm, wref.SNRS[lv], name, dg[m].max(), df[m].max(), bound.min()))
                    if not ratio <= 1.0:
                        fails.append((nharm, ndm, wref.SNRS[lv], name, round(ratio, 2)))
    print("nbin %d: evaluations max %d; worst distance / bound per column %s"
          % (nbin, nev_max, {k: round(v, 3) for k, v in worst.items()}))
    assert not fails, fails


@pytest.mark.parametrize("nbin", (256, 97))
def test_same_bits_in_every_layout_and_run(nbin, hip_lib):
    nharm = wref.nharms(nbin)[1]
    cb = wref.eval_block(ref.harmonics(nbin, nharm))[1]
    c = wref.case_inputs(nbin, cb + 1, 5, True, nharm, 5)
    ld = (5 * nbin + 7) // 4 * 4
    base = run_wide(hip_lib, c, ld=ld, out_ld=12, prof_ld=4)
    for lay in (dict(ld=ld, out_ld=12, prof_ld=4), dict(ld=kh.odd(ld), in_off=1, out_ld=11, out_off=1, prof_ld=5, prof_off=1),
                dict(ld=ld, in_off=1), dict(ld=kh.odd(ld)), dict(ld=5 * nbin, out_ld=10, prof_ld=4),
                dict(work_off=1, prof_ld=7, prof_off=3)):
        got = run_wide(hip_lib, c, **lay)
        assert same_bits(base[0], got[0]) and same_bits(base[1], got[1]), lay


@pytest.mark.parametrize("nbin", (256, 50))
def test_a_sub_integration_does_not_depend_on_its_neighbours(nbin, hip_lib):
    """Every sub-integration of a batch fitted alone gives the bits it has inside the batch."""
    nharm, nchan, nsub = nbin, 5, 5
    c = wref.case_inputs(nbin, nchan, nsub, True, nharm, 5)
    out, rows = run_wide(hip_lib, c)
    for s in range(nsub):
        one = dict(c, profiles=np.ascontiguousarray(c["profiles"][:, s:s + 1]), wt=np.ascontiguousarray(c["wt"][:, s:s + 1]))
        o1, r1 = run_wide(hip_lib, one)
        assert same_bits(o1[0], out[s]) and same_bits(r1[:, 0], rows[:, s]), s


@pytest.mark.parametrize("nbin", (256, 97))
def test_channels_left_out(nbin, hip_lib):
    """A zero-weight channel and a channel with a NaN are left out and
    reported, and the result is, bit for bit, the fit of the channels that
    remain -- here across an evaluation block's boundary."""
    nharm = wref.nharms(nbin)[1]
    cb = wref.eval_block(ref.harmonics(nbin, nharm))[1]
    nchan, nsub = cb + 3, 2
    c = wref.case_inputs(nbin, nchan, nsub, True, nharm, 1)
    prof, wt = c["profiles"].copy(), c["wt"].copy()
    prof[1, :, nbin // 3] = np.nan
    wt[cb - 1, :] = 0.0
    wt[2, 1] = -1.0                                            # in the second sub-integration alone
    full, _ = run_wide(hip_lib, c)
    out, rows = run_wide(hip_lib, dict(c, profiles=prof, wt=wt))
    assert list(out[:, wref.NUSED]) == [nchan - 2, nchan - 3] and not out[:, wref.STATUS].any()
    K = ref.harmonics(nbin, nharm)
    assert list(out[:, wref.DOF]) == [(2 * K - 1) * (nchan - 2) - 2, (2 * K - 1) * (nchan - 3) - 2]
    assert list(full[:, wref.NUSED]) == [nchan, nchan]
    gone = [(1, 0), (1, 1), (cb - 1, 0), (cb - 1, 1), (2, 1)]
    for ch, s in gone:
        assert rows[ch, s, 3] == 0 and rows[ch, s, 2] == 0 and np.isinf(rows[ch, s, 1])
        assert np.isnan(rows[ch, s, 0]) if ch == 1 else rows[ch, s, 0] == 0
    assert rows[:, :, 3].sum() == 2 * nchan - 5
    for s, drop in ((0, (1, cb - 1)), (1, (1, 2, cb - 1))):
        keep = [ch for ch in range(nchan) if ch not in drop]
        rest = dict(c, profiles=np.ascontiguousarray(c["profiles"][keep, s:s + 1]), wt=np.ascontiguousarray(c["wt"][keep, s:s + 1]),
                    spec=np.ascontiguousarray(c["spec"][keep]), kappa=c["kappa"][keep], phi0=c["phi0"][keep])
        o2, r2 = run_wide(hip_lib, rest)
        assert same_bits(o2[0], out[s]) and same_bits(r2[:, 0], np.ascontiguousarray(rows[keep, s])), s


def test_degenerate_sub_integrations(hip_lib):
    """One usable channel, and no usable channel at all: status 2, errors +inf,
    no evaluation -- as the model has them -- next to an ordinary
    sub-integration that keeps its bits."""
    nbin, nharm = 256, 63
    c = wref.case_inputs(nbin, 5, 3, True, nharm, 5)
    plain, _ = run_wide(hip_lib, c)
    wt = c["wt"].copy()
    wt[:, 0] = 0.0
    wt[[0, 1, 3, 4], 2] = np.nan
    bad = dict(c, wt=wt)
    out, rows = run_wide(hip_lib, bad)
    want, wrows = wref.wide_ref(*wref.model_args(bad))
    assert same_bits(out[1], plain[1])
    assert list(out[:, wref.STATUS]) == list(want[:, wref.STATUS]) == [2, 0, 2]
    assert list(out[:, wref.NUSED]) == [0, 5, 1] and list(out[:, wref.NEV][[0, 2]]) == [0, 0]
    for s in (0, 2):
        assert np.isinf(out[s, [wref.PHI_ERR, wref.D_ERR]]).all() and out[s, wref.COV] == 0 and out[s, wref.D] == want[s, wref.D]
        assert out[s, wref.DOF] == want[s, wref.DOF]
    assert np.array_equal(rows[:, :, 3], wrows[:, :, 3]) and rows[2, 2, 3] == 1 and not rows[:, 0, 3].any()
    assert abs(ref.circ(out[2, wref.PHI] - want[2, wref.PHI])) < 1.0 / nbin         # (the coarse start)
    one = dict(c, profiles=c["profiles"][:1], wt=c["wt"][:1], spec=c["spec"][:1], kappa=c["kappa"][:1], phi0=c["phi0"][:1])
    o1, _ = run_wide(hip_lib, one)
    assert (o1[:, wref.STATUS] == 2).all() and np.isinf(o1[:, wref.PHI_ERR]).all()
    same = dict(c, kappa=np.full(5, 3.0))
    o2, _ = run_wide(hip_lib, same)
    assert (o2[:, wref.STATUS] == 2).all() and np.isinf(o2[:, wref.D_ERR]).all()


def test_backend_fit_wideband_is_the_entry_point(hip_lib):
    import torch
    from psrsigsim_amd.telescope import Backend
    nbin, nchan, nsub = 256, 5, 5
    c = wref.case_inputs(nbin, nchan, nsub, True, 40, 5)
    tm = np.stack([ref.make_template(nbin, ("multi", "inter")[ch % 2]) * (1 + ch / 4) for ch in range(nchan)])
    t = Backend.toa_template(tm, nbin, nharm=40)
    assert np.array_equal(t.spec, c["spec"])
    data = torch.from_numpy(c["profiles"].reshape(nchan, nsub * nbin)).cuda()
    out, rows = Backend(samprate=0.01).fit_wideband(data, nchan, nsub, nbin, t, c["kappa"], c["phi0"], c["wt"],
                                                    ndm=5, dm_step=c["dm_step"])
    assert tuple(out.shape) == (nsub, 10) and out.dtype == torch.float64
    assert tuple(rows.shape) == (nchan, nsub, 4) and rows.dtype == torch.float32
    want = run_wide(hip_lib, c)
    assert same_bits(out.cpu().numpy(), want[0]) and same_bits(rows.cpu().numpy(), want[1])
    out2, _ = Backend(samprate=0.01).fit_wideband(data, nchan, nsub, nbin, t, torch.from_numpy(c["kappa"]).cuda(),
                                                  torch.from_numpy(c["phi0"]), torch.from_numpy(c["wt"]).cuda(), 5,
                                                  c["dm_step"])
    assert same_bits(out2.cpu().numpy(), want[0])


def test_stages_are_the_fit_in_parts(hip_lib):
    """pss_toa_wide_stages 0 .. 1, 2 and 3 on one workspace leave what pss_toa_wide_fit leaves."""
    import torch
    nbin, nchan, nsub = 256, 5, 5
    c = wref.case_inputs(nbin, nchan, nsub, True, 63, 5)
    want = run_wide(hip_lib, c)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()      # noqa: E731
    data, spec, wt = dev(c["profiles"].reshape(nchan, -1), np.float32), dev(c["spec"], np.float32), dev(c["wt"], np.float32)
    kap, ph0 = dev(c["kappa"], np.float64), dev(c["phi0"], np.float64)
    need = int(hip_lib.pss_toa_wide_workspace_bytes(nchan, nsub, nbin, 63, 5))
    work = torch.zeros((need,), dtype=torch.uint8, device="cuda")
    out = torch.zeros((nsub, 10), dtype=torch.float64, device="cuda")
    rows = torch.zeros((nchan, nsub, 4), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    for first, last in ((0, 1), (2, 2), (3, 3)):
        rc = hip_lib.pss_toa_wide_stages(data.data_ptr(), nchan, nsub, nbin, nsub * nbin, spec.data_ptr(), nchan, 63,
                                         kap.data_ptr(), ph0.data_ptr(), wt.data_ptr(), 5, float(c["dm_step"]),
                                         out.data_ptr(), 10, rows.data_ptr(), 4, work.data_ptr(), need, first, last, None)
        assert rc == 0, (first, last)
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), want[0]) and same_bits(rows.cpu().numpy(), want[1])


def _fold_signal(seed, dm, smean=2e-4):
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar, GaussProfile
    from psrsigsim_amd.ism import ISM
    from psrsigsim_amd.telescope import Backend, Receiver, telescope as T
    P, nfold = 0.004, 10000                                    # 256 bins at 64 kHz
    pss.seed(seed)
    sig = FilterBankSignal(1400, 400, Nsubband=8, sample_rate=0.064, sublen=P * nfold, fold=True)
    psr = Pulsar(P, smean, profiles=GaussProfile(0.5, 0.05, 1))
    psr.make_pulses(sig, tobs=4 * P * nfold)
    ISM().disperse(sig, dm)
    tel = T.Arecibo()
    # equal rates: the backend's 1 / (2 samprate) is the signal's sublen / nbin
    tel.add_system(name="S", receiver=Receiver(fcent=1400, bandwidth=400, name="L"),
                   backend=Backend(samprate=0.064 / (2 * nfold), name="B"))
    assert T.Telescope.resample_branch(sig, tel.systems["S"][1])[0] == "copy"
    tel.observe(sig, psr, system="S", noise=True)
    return sig, psr, P


def test_wideband_toas_close_the_loop_on_an_injected_dm(hip_lib):
    """The signal of test_gpu_toa.py's end-to-end test (8 channels x 4
    sub-integrations of 256 bins, DM 0.3, narrowband b / b_err 55): the
    wideband DM of every sub-integration lies within 5 dm_err of 0.3, and
    their weighted mean within the narrowband ``fit_dm`` +- its error.  (The
    CPU oracle's signal under the float64 model, seeds 11, 12, 13: largest DM
    pull of a sub-integration 1.42, 2.06 and 0.58; weighted mean against
    fit_dm 0.30159 / 0.30157, 0.30023 / 0.30016, 0.29907 / 0.29908, the
    latter +- 0.0022.)"""
    from psrsigsim_amd.telescope import Backend, WidebandTOAs
    dm0 = 0.3
    sig, psr, P = _fold_signal(11, dm0)
    be = Backend(samprate=0.064)
    t = be.wideband_toas(sig, psr)
    assert isinstance(t, WidebandTOAs) and t.shift.shape == (4,) and t.period == P and t.sublen == 40.0
    assert t.scale.shape == (8, 4) and t.used.all() and (t.nchan_used == 8).all() and t.dm_nominal == dm0
    pull = (t.dm - dm0) / t.dm_err
    nb_dm, nb_err, _ = be.toas(sig, psr).fit_dm()
    mean = float((t.dm / t.dm_err ** 2).sum() / (1.0 / t.dm_err ** 2).sum())
    print("dm %s +- %s (pulls %s), evaluations %s, chi2r %s; weighted mean %.5f, narrowband %.5f +- %.5f; ref_freq %s"
          % (np.round(t.dm, 5), np.round(t.dm_err, 5), np.round(pull, 2), t.nev, np.round(t.chi2r, 3), mean, nb_dm, nb_err,
             np.round(t.ref_freq, 1)))
    assert not t.status.any()
    assert (np.abs(pull) <= 5).all() and (t.dm_err < 0.01).all()
    assert abs(mean - nb_dm) <= nb_err
    assert ((t.ref_freq > 1200) & (t.ref_freq < 1600)).all() and (t.shift_ref_err < t.shift_err).all()
    # a nominal DM that is off by three error bars is found again, with the trials to start from
    t2 = be.wideband_toas(sig, psr, dm=dm0 + 0.012, ndm=5)
    assert not t2.status.any() and np.abs(t2.dm - t.dm).max() <= 0.1 * t.dm_err.min()


def test_wideband_toas_at_low_signal(hip_lib):
    """The same observation with the pulsar 18 x fainter, so that the
    narrowband b / b_err has a median of about 3 and FFTFIT's coarse maximum
    starts to pick noise peaks: the wideband DM still lies within 5 dm_err of
    the injected 0.3 in every sub-integration, and ``shift_ref`` within 5
    shift_ref_err of the injected delay at ``ref_freq`` (0: the nominal DM is
    the injected one).  (The CPU oracle's signal under the float64 model, seeds
    11, 12, 13: narrowband median 2.94, 3.25, 3.07; largest DM pull 1.51, 1.95,
    1.13; largest shift_ref pull 0.30, 1.28, 2.09; status 0 in all twelve
    sub-integrations within 9 evaluations.)"""
    from psrsigsim_amd.telescope import Backend
    dm0 = 0.3
    sig, psr, P = _fold_signal(11, dm0, smean=1.1e-5)
    be = Backend(samprate=0.064)
    snr = float(np.median(be.toas(sig, psr).snr))
    t = be.wideband_toas(sig, psr)
    pull = (t.dm - dm0) / t.dm_err
    rpull = ref.circ(t.shift_ref) / t.shift_ref_err
    print("narrowband snr median %.2f; dm %s +- %s (pulls %s); shift_ref pulls %s; evaluations %s; status %s"
          % (snr, np.round(t.dm, 4), np.round(t.dm_err, 4), np.round(pull, 2), np.round(rpull, 2), t.nev, t.status))
    assert 2.0 <= snr <= 4.5
    assert not t.status.any()
    assert (np.abs(pull) <= 5).all() and (np.abs(rpull) <= 5).all()


def test_wideband_toas_rejections(hip_lib):
    from psrsigsim_amd.telescope import Backend
    be = Backend(samprate=0.064)
    sig, psr, _ = _fold_signal(3, 0.1)
    with pytest.raises(ValueError, match="needs a pulsar or a template"):
        be.wideband_toas(sig)
    with pytest.raises(ValueError, match="ndm 2 is not odd"):
        be.wideband_toas(sig, psr, ndm=2)
    sig._nsub = 3
    with pytest.raises(ValueError, match="3 sub-integrations do not divide a row of 1024 samples"):
        be.wideband_toas(sig, psr)
