"""The device's random draws against the float64 stream definition
(tests/philox_ref.py), draw for draw: pss_chi2_fill (the chi2(1) sampler and
the Marsaglia-Tsang pair sampler with its retries and boost), the keying
invariants, pss_normal_add (the Box-Muller normals), and the pipeline itself
-- a Philox-mode run against the same run with the model's draws injected.

Bounds.  The device evaluates log, cos, sin and exp2 with the hardware's
approximations, whose error nobody has tabulated here, so the relative bounds
are measured: one run over all cases gave the largest ratios

  TAU1  chi2(1), |dev - model| / h                 3.88e-7  ->  TAU1 = 3.11e-6
  TAU   pair sampler, |dev - model| / model        5.44e-6  ->  TAU  = 4.35e-5
  TAUN  normals, |dev - scale z| / (scale l)       2.08e-7  ->  TAUN = 1.66e-6

and each bound is 8 x its measured maximum (one run samples only part of the
argument range).  A measured TAU1 or TAU above 1e-4, or TAUN above 1e-5,
would mean a wrong formula, not rounding (asserted).  Per-case figures are in
profiles/draw_streams/README.md.

A pair-sampler draw whose decision margin (philox_ref.chi2_rows) is below
EPS = 1e-3 is undecided and not compared: fp32 and float64 may settle such an
accept differently and the value then comes from another block.  EPS is a
condition on the draw, not a tolerance on the value; at most 0.5 % of a case
may be undecided, every other draw must match."""
import numpy as np
import pytest
import torch

from tests import philox_ref as R
from tests import replay

pytestmark = pytest.mark.gpu

TAU1 = 8 * 3.883e-7
TAU = 8 * 5.437e-6
TAUN = 8 * 2.076e-7
# what a measured maximum may not exceed: above it the formula is wrong
TAU1_MAX, TAU_MAX, TAUN_MAX = 1e-4, 1e-4, 1e-5
ULP = 2.0 ** -24
SEED = R.FILL_SEED


@pytest.fixture(autouse=True)
def _engine_state_restored():
    """Seed, call counter, flags and injections back, pass or fail."""
    from psrsigsim_amd import _engine, _lib
    saved = dict(_engine._state)
    flags = _lib.lib().pss_set_flags(0)
    _lib.lib().pss_set_flags(flags)
    try:
        yield
    finally:
        _engine._state.update(saved)
        _engine.clear_injections()
        _lib.lib().pss_set_flags(flags)


def _fill(rows, chan0, n, df, call, purpose, seed=SEED):
    from psrsigsim_amd import _lib, _engine
    out = torch.full((rows, n), float("nan"), dtype=torch.float32, device="cuda")
    rc = _lib.lib().pss_chi2_fill(_engine.ptr(out), rows, chan0, n, float(df), seed, call, purpose,
                                  _engine.stream_ptr())
    _lib.check(rc)
    return out.cpu().numpy()


# ---------------------------------------------------------------------------
# (a) pss_chi2_fill against the model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("df,chan0,call,purpose", R.fill_cases(),
                         ids=["df%g-c%d-call%x-p%d" % c for c in R.fill_cases()])
def test_chi2_fill_matches_model(df, chan0, call, purpose, hip_lib):
    x, depth, margin, h, counts = R.fill_model(df, chan0, call, purpose)
    R.check_fill_counts(df, counts)
    dev = _fill(R.FILL_ROWS, chan0, R.FILL_N, df, call, purpose).astype(np.float64)
    assert np.isfinite(dev).all()
    if df == 1.0:
        ratio = np.abs(dev - x) / np.maximum(h, 1e-300)     # (h = 0, u = 1: both sides 0)
        worst, bound, cap = float(ratio.max()), TAU1, TAU1_MAX
    else:
        decided = margin >= R.EPS
        ratio = np.where(decided, np.abs(dev - x) / x, 0.0)
        worst, bound, cap = float(ratio.max()), TAU, TAU_MAX
    print("fill df=%g chan0=%d call=%#x purpose=%d: worst ratio %.3e, %s" % (df, chan0, call, purpose, worst, counts))
    assert worst <= cap, "a ratio of %.3g is a wrong formula, not rounding" % worst
    assert worst <= bound, (worst, bound, np.unravel_index(np.argmax(ratio), ratio.shape))


# ---------------------------------------------------------------------------
# (b) keying invariants, device only, bitwise
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("df", [1.0, 3.7])
def test_fill_keying_invariants(df, hip_lib):
    full = _fill(8, 0, R.FILL_N, df, 1, R.P_TEST)
    # a shorter fill is a prefix (its ragged tail comes from the same blocks)
    np.testing.assert_array_equal(_fill(8, 0, 1001, df, 1, R.P_TEST), full[:, :1001])
    # rows are keyed by GLOBAL channel
    np.testing.assert_array_equal(_fill(3, 5, R.FILL_N, df, 1, R.P_TEST), full[5:8])
    # ... and no two channels draw the same values (a key that ignored the channel would pass the line above)
    assert len({row.tobytes() for row in full}) == 8


# ---------------------------------------------------------------------------
# (c) pss_normal_add against the model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("offset,ld", [(0, 4104), (1, 4101)], ids=["grid16", "misaligned"])
def test_normal_add_matches_model(offset, ld, hip_lib):
    from psrsigsim_amd import _lib, _engine
    rows, n, scale, call, pad = 3, R.FILL_N, 0.75, 3, 7.0
    host = np.full(offset + rows * ld + 8, pad, dtype=np.float32)
    view = host[offset:offset + rows * ld].reshape(rows, ld)
    view[:, :n] = 0.0
    flat = torch.from_numpy(host).cuda()
    assert flat.data_ptr() % 16 == 0
    rc = _lib.lib().pss_normal_add(_engine.ptr(flat[offset:]), rows, n, ld, scale, SEED, call, _engine.stream_ptr())
    _lib.check(rc, "normal_add")
    got = flat.cpu().numpy()
    gv = got[offset:offset + rows * ld].reshape(rows, ld)
    z, l = R.normal_rows(rows, 0, n, SEED, call, R.P_NOISE)
    ratio = np.abs(gv[:, :n].astype(np.float64) - scale * z) / np.maximum(scale * l, 1e-300)
    worst = float(ratio.max())
    print("normal_add offset=%d ld=%d: worst ratio %.3e" % (offset, ld, worst))
    assert worst <= TAUN_MAX, "a ratio of %.3g is a wrong formula, not rounding" % worst
    assert worst <= TAUN, (worst, TAUN)
    # nothing outside the rows' n columns is touched
    untouched = np.ones(got.shape, dtype=bool)
    for r in range(rows):
        untouched[offset + r * ld: offset + r * ld + n] = False
    assert (got[untouched].view(np.uint32) == np.float32(pad).view(np.uint32)).all()


# ---------------------------------------------------------------------------
# (d) the pipeline draws the model's values
# ---------------------------------------------------------------------------
def _three_runs(run, nchan, n, gen, noise):
    """run(inj) for inj = None (Philox), the model's draws, and (ones, zeros):
    the Philox run, the injected run and the factor P the source stage puts on
    a pulse draw (profile x norm, as the device evaluates it)."""
    import psrsigsim_amd as pss
    out = []
    for inj in (None, dict(gen=gen, noise=noise)):
        pss.seed(SEED)
        if inj is not None:
            pss.inject(**inj)
        try:
            out.append(run())
        finally:
            pss._engine.clear_injections()
    return out + [(_profile_factor(run, nchan, n), None)]


def _profile_factor(run, nchan, n):
    import psrsigsim_amd as pss
    pss.seed(SEED)
    pss.inject(gen=np.ones((nchan, n), np.float32), noise=np.zeros((nchan, n), np.float32))
    try:
        return run()[0]
    finally:
        pss._engine.clear_injections()


def _search(nchan, n, dm):
    def run():
        from psrsigsim_amd.signal import FilterBankSignal
        from psrsigsim_amd.pulsar import Pulsar, GaussProfile
        from psrsigsim_amd.ism import ISM
        from psrsigsim_amd.telescope import telescope as T
        from psrsigsim_amd.telescope.receiver import Receiver
        sig = FilterBankSignal(1400, 400, Nsubband=nchan, fold=False)
        psr = Pulsar(0.005, 1.0, profiles=GaussProfile(0.5, 0.05, 1))
        psr.make_pulses(sig, tobs=(n + 0.5) * 20.48e-6)              # call 1
        assert sig.nsamp == n
        if dm:
            ISM().disperse(sig, dm)
        tel = T.Arecibo()
        tel.observe(sig, psr, system="Lband_PUPPI", noise=True)      # call 2
        return sig.data.cpu().numpy().astype(np.float64), float(Receiver.noise_norm(sig, psr, tel.Tsys, tel.gain))
    return run


def test_search_pipeline_draws_model_values(hip_lib):
    """3 x 4096, no delay: out = P x_pulse + norm x_noise elementwise.  Bound:
    TAU1 (P h_pulse + norm h_noise), the draw bound of the fill test through
    the two products, plus ten fp32 roundings (the scale folded into the
    sampler or applied to the injected fp32 value, the profile product, the
    noise multiply-add, on either side), each relative to a term that is at
    most P 2 h_pulse + norm 2 h_noise."""
    nchan, n = 3, 4096
    gx, _, gm, gh = R.chi2_rows(nchan, 0, n, 1.0, SEED, 1, R.P_PULSE)
    nx, _, nm, nh = R.chi2_rows(nchan, 0, n, 1.0, SEED, 2, R.P_NOISE)
    undecided = (gm < R.EPS) | (nm < R.EPS)
    assert undecided.mean() <= R.UNDECIDED_CAP
    (a, norm), (b, _), (P, _) = _three_runs(_search(nchan, n, 0), nchan, n, gx, nx)
    assert P.max() > 0 and norm > 0
    bound = TAU1 * (P * gh + norm * nh) + 10 * ULP * 2 * (P * gh + norm * nh)
    ratio = np.where(undecided, 0.0, np.abs(a - b) / bound)
    print("search 3x4096: worst |run1 - run2| / bound %.3f" % ratio.max())
    assert ratio.max() <= 1.0, (ratio.max(), np.unravel_index(np.argmax(ratio), ratio.shape))


@pytest.mark.parametrize("no_fast", [False, True], ids=["fast", "generic"])
def test_delayed_search_pipeline_draws_model_values(no_fast, hip_lib):
    """4 x 2^14 at DM 100 (the smallest four-step length, pair rows): the
    Philox run on the fast passes A and C, or on the generic ones under
    PSS_FLAG_NO_FAST, against the run with the model's draws injected (the
    generic passes: injection is their business).  The delay is a circular
    fractional shift, linear, its kernel's L1 norm (the Dirichlet kernel's
    Lebesgue constant) at most 4/pi^2 ln N + 2; so per row, relative to the
    row maximum, the runs differ by at most that times the largest pulse-draw
    bound TAU1 P h, plus the noise-draw bound TAU1 norm h, plus the fp32
    transform's own error on either run, 1e-5 each (the parity gate of every
    delay test here).  chi2(1) draws have no undecided values."""
    from psrsigsim_amd import _lib
    nchan, n = 4, 1 << 14
    gx, _, gm, gh = R.chi2_rows(nchan, 0, n, 1.0, SEED, 1, R.P_PULSE)
    nx, _, nm, nh = R.chi2_rows(nchan, 0, n, 1.0, SEED, 2, R.P_NOISE)
    assert not ((gm < R.EPS) | (nm < R.EPS)).any()
    import psrsigsim_amd as pss
    run = _search(nchan, n, 100)
    fast, generic = ("A:fast_shared", "C:fast"), ("A:generic", "C:generic")   # (one profile row for all channels)
    L = _lib.lib()
    old = L.pss_set_flags(_lib.FLAG_NO_FAST) if no_fast else None
    try:
        pss.seed(SEED)
        _lib.plan_collect()
        a, norm = run()
        replay.assert_plan(_lib.plan_collect(), nchan, n, ("fourstep", "16x1024") + (generic if no_fast else fast),
                           absent=fast if no_fast else generic)
        pss.seed(SEED)
        pss.inject(gen=gx, noise=nx)
        b, _ = run()
    finally:
        pss._engine.clear_injections()
        if old is not None:
            L.pss_set_flags(old)
    # P: the undelayed profile factor (a delay moves it, its maximum stays)
    P = _profile_factor(_search(nchan, n, 0), nchan, n)
    l1 = 4.0 / np.pi ** 2 * np.log(n) + 2.0
    rowmax = np.abs(b).max(axis=1)
    bound = (l1 * TAU1 * (P * gh).max(axis=1) + TAU1 * norm * nh.max(axis=1)) / rowmax + 2e-5
    err = np.abs(a - b).max(axis=1) / rowmax
    print("search 4x2^14 DM 100 (%s): |run1 - run2| / rowmax %s, bound %s" % ("generic" if no_fast else "fast", err, bound))
    assert (err <= bound).all(), (err, bound)


F0_B1855 = 186.4940812499314404


def test_fold_pipeline_draws_model_values(hip_lib):
    """Fold mode, 3 channels x 6144 (six 1024-bin subintegrations: a 6 x 1024
    mixed-radix length), no delay: pulse and noise draws are chi2(Nfold),
    Nfold = 11189.6, the Marsaglia-Tsang pair path.  Elementwise, bound
    TAU (P x_pulse + norm x_noise) plus ten fp32 roundings of those terms.
    At this df about 1e-3 of all draws are undecided whatever the seed (the
    accept test of a draw with u > 1 - EPS is within EPS of its boundary), so
    no seed leaves the 36864 draws of this shape free of them; they are masked
    out under the same 0.5 % cap as in the fill test."""
    nchan, nbin, nsub = 3, 1024, 6
    n = nbin * nsub

    def run():
        from psrsigsim_amd.signal import FilterBankSignal
        from psrsigsim_amd.pulsar import Pulsar, GaussProfile
        from psrsigsim_amd.telescope import telescope as T
        from psrsigsim_amd.telescope.receiver import Receiver
        sig = FilterBankSignal(1400, 400, Nsubband=nchan, sample_rate=F0_B1855 * nbin * 1e-6, sublen=60.0, fold=True)
        psr = Pulsar(1.0 / F0_B1855, 0.005, profiles=GaussProfile(0.5, 0.05, 1))
        psr.make_pulses(sig, tobs=60.0 * nsub)                        # call 1
        tel = T.Arecibo()
        tel.observe(sig, psr, system="Lband_PUPPI", noise=True)      # call 2
        d = sig.data.cpu().numpy().astype(np.float64)
        assert d.shape == (nchan, n)
        return d, (float(Receiver.noise_norm(sig, psr, tel.Tsys, tel.gain)), float(sig.Nfold))

    df = float(np.float32(60.0 * F0_B1855))
    gx, gd, gm, _ = R.chi2_rows(nchan, 0, n, df, SEED, 1, R.P_PULSE)
    nx, nd, nm, _ = R.chi2_rows(nchan, 0, n, df, SEED, 2, R.P_NOISE)
    undecided = (gm < R.EPS) | (nm < R.EPS)
    assert undecided.mean() <= R.UNDECIDED_CAP
    (a, (norm, nfold)), (b, _), (P, _) = _three_runs(run, nchan, n, gx, nx)
    assert abs(nfold - df) <= 1e-3 and df != 1.0
    assert P.max() > 0 and norm > 0
    bound = (TAU + 10 * ULP) * (P * gx + norm * nx)
    ratio = np.where(undecided, 0.0, np.abs(a - b) / bound)
    print("fold 3x6144 df=%.1f: worst |run1 - run2| / bound %.3f, undecided %.2e" % (df, ratio.max(), undecided.mean()))
    assert ratio.max() <= 1.0, (ratio.max(), np.unravel_index(np.argmax(ratio), ratio.shape))


def test_baseband_pipeline_draws_model_values(hip_lib):
    """One BasebandSignal, 2 x 4099: amplitude pulses sqrt(profile) x N(0, 1)
    (purpose 1, keyed by channel) and amplitude noise norm x N(0, 1)
    (pss_normal_add, purpose 4, keyed by row).  The amplitude noise takes no
    injection, so the second run injects the model's pulse normals and adds
    norm x the model's noise normals on the host in float64.  Bound:
    TAUN (P l_pulse + norm l_noise) plus ten fp32 roundings of those terms."""
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import BasebandSignal
    from psrsigsim_amd.pulsar import Pulsar, GaussProfile
    from psrsigsim_amd.telescope import Receiver
    nchan, n, bw, tsys = 2, R.FILL_N, 0.512, 100.0
    gz, gl = R.normal_rows(nchan, 0, n, SEED, 1, R.P_PULSE)
    nz, nl = R.normal_rows(nchan, 0, n, SEED, 2, R.P_NOISE)

    def run(inj, noise):
        pss.seed(SEED)
        if inj is not None:
            pss.inject(gen=inj)
        try:
            bb = BasebandSignal(1400, bw, Nchan=nchan)
            psr = Pulsar(0.004, 1e-5, profiles=GaussProfile(0.5, 0.05, 1), name="J0000+0000")   # 4096 samples a period
            psr.make_pulses(bb, (n + 0.5) / 1.024e6)                                 # call 1
            assert bb.nsamp == n
            norm = Receiver.amp_noise_norm(bb, psr, tsys, 1.0)
            if noise:
                Receiver(fcent=1400, bandwidth=bw, name="L").radiometer_noise(bb, psr, gain=1.0, Tsys=tsys)   # call 2
            return bb.data.cpu().numpy().astype(np.float64), norm
        finally:
            pss._engine.clear_injections()

    a, norm = run(None, True)
    b, _ = run(gz, False)
    b = b + norm * nz
    P, _ = run(np.ones((nchan, n), np.float32), False)
    assert P.max() > 0.5 and norm > 0
    bound = (TAUN + 10 * ULP) * (P * gl + norm * nl)
    ratio = np.abs(a - b) / bound
    print("baseband 2x4099: worst |run1 - run2| / bound %.3f" % ratio.max())
    assert ratio.max() <= 1.0, (ratio.max(), np.unravel_index(np.argmax(ratio), ratio.shape))
