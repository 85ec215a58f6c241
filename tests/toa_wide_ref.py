"""The float64 model of the wideband fit ``pss_toa_wide_fit`` (include/pss_hip.h),
its single-precision restatement, and the inputs the wideband tests share.

* ``wide_ref``  -- the model: NumPy ``rfft`` in float64, the coarse start over
  the DM trials, then the safeguarded Newton iteration on (phi, d) with the
  step, acceptance and stopping rules of the header, step for step.
* ``wide_f32``  -- the same steps with complex64 spectra from SciPy's
  single-precision transform and float32 harmonic sums; the phase reduction and
  everything per channel and above stay float64, as in the kernel.  The GPU
  tests take their tolerance from its distance to the model.
* ``near_tie``  -- per sub-integration: at the chosen DM trial the model's two
  highest distinct local maxima of the coarse correlation lie within 1e-3 of
  the maximum of each other.
* ``case_inputs``, ``low_signal``, ``all_cases`` and the shape tables -- inputs.
"""
import numpy as np

from tests import toa_ref as ref

COLS = ("phi", "phi_err", "d", "d_err", "cov", "chi2", "dof", "nused", "nev", "status")
PHI, PHI_ERR, D, D_ERR, COV, CHI2, DOF, NUSED, NEV, STATUS = range(10)
TWO_PI = 2.0 * np.pi
EVALS = 32
TOL = 2.0 ** -26
CLAMP_BINS = 4.0


def eval_block(K):
    """(lanes of a channel's group, usable channels of an evaluation block) at K harmonics."""
    G = 64 if K > 32 else (16 if K > 8 else 4)
    return G, 256 // G


def _spectra(profs, spec, nharm, single):
    """X [nchan, nsub, K] and PP, S2, T2 [nchan, nsub] (T2, S2 per channel), finite [nchan, nsub]."""
    dt = np.float32 if single else np.float64
    ct = np.complex64 if single else np.complex128
    p = np.asarray(profs).astype(dt)
    nchan, nsub, N = p.shape
    K = ref.harmonics(N, nharm)
    spec = np.asarray(spec, dtype=np.float32)
    assert spec.shape[-2:] == (K + 1, 2) and spec.shape[0] in (1, nchan)
    S = (spec[..., 0].astype(dt) + 1j * spec[..., 1].astype(dt)).astype(ct)
    S = np.broadcast_to(S, (nchan, K + 1))[:, None, 1:]
    finite = np.isfinite(p).all(axis=2)
    p0 = np.where(finite, p[:, :, 0], dt(0))
    pz = np.where(finite[:, :, None], p - p0[:, :, None], dt(0))
    if single:
        import scipy.fft
        P = scipy.fft.rfft(pz, axis=2)
        assert P.dtype == np.complex64
    else:
        P = np.fft.rfft(pz, axis=2)
    Pk = P[:, :, 1:K + 1]
    X = Pk * np.conj(S)
    s2 = (S.real * S.real + S.imag * S.imag)
    S2 = s2.sum(axis=2, dtype=np.float64)[:, 0]
    k = np.arange(1, K + 1, dtype=np.float64)
    T2 = (s2.astype(np.float64) * k * k).sum(axis=2)[:, 0]
    PP = (Pk.real * Pk.real + Pk.imag * Pk.imag).sum(axis=2, dtype=np.float64)
    return X.astype(ct), PP, S2, T2, finite, K


def _turn(k, ph, single):
    """e^{2 pi i k ph}: the product in float64, reduced, then rounded to the working precision."""
    t = k[None, :] * ph[:, None]
    t = t - np.rint(t)
    if single:
        a = (np.float32(TWO_PI) * t.astype(np.float32)).astype(np.float32)
        return (np.cos(a) + 1j * np.sin(a)).astype(np.complex64)
    a = TWO_PI * t
    return np.cos(a) + 1j * np.sin(a)


def _newton(S, kspan, nbin):
    h11, h12, h22 = S[2], S[3], S[4]
    det = h11 * h22 - h12 * h12
    if not (h11 < 0 and det > 0):
        h11, h12, h22 = S[5], S[6], S[7]
        det = h11 * h22 - h12 * h12
    if not (h11 < 0 and det > 0):
        return 0.0, 0.0
    pp = -(h22 * S[0] - h12 * S[1]) / det
    pd = -(h11 * S[1] - h12 * S[0]) / det
    ln = max(abs(pp), abs(pd) * kspan) * nbin / CLAMP_BINS
    if ln > 1:
        pp, pd = pp / ln, pd / ln
    if not (np.isfinite(pp) and np.isfinite(pd)):
        return 0.0, 0.0
    return pp, pd


def _fit(profs, spec, nharm, kappa, phi0, wt, ndm, dm_step, single):
    X, PP, S2, T2, finite, K = _spectra(profs, spec, nharm, single)
    nchan, nsub, N = np.shape(profs)
    st = np.float32 if single else np.float64
    kappa = np.asarray(kappa, dtype=np.float64)
    phi0 = np.asarray(phi0, dtype=np.float64)
    wt = np.asarray(wt, dtype=np.float32)
    assert wt.shape == (nchan, nsub) and ndm >= 1 and ndm % 2 == 1
    k = np.arange(1, K + 1, dtype=np.float64)
    kf = k.astype(st)
    out = np.zeros((nsub, 10))
    prof = np.zeros((nchan, nsub, 4))
    tie = np.zeros(nsub, dtype=bool)
    for s in range(nsub):
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(wt[:, s]) & (wt[:, s] > 0) & finite[:, s] & (S2 > 0)
        bad = ~ok
        prof[bad, s] = np.stack([np.where(finite[bad, s], 0.0, np.nan), np.full(bad.sum(), np.inf),
                                 np.zeros(bad.sum()), np.zeros(bad.sum())], axis=1)
        u = np.flatnonzero(ok)
        n = u.size
        Xs, w64, kap, p0s = X[u, s], wt[u, s].astype(np.float64), kappa[u], phi0[u]
        S2u, T2u, PPu = S2[u], T2[u], PP[u, s]
        kbar = kap.sum() / n if n else 0.0
        kspan = max(kap.max() - kbar, kbar - kap.min()) if n else 0.0

        def ev(phi, d):
            ph = p0s + phi + kap * d
            ph = ph - np.rint(ph)
            Z = Xs * _turn(k, ph, single)
            C = Z.real.sum(axis=1, dtype=st).astype(np.float64)
            g = (kf * Z.imag).sum(axis=1, dtype=st).astype(np.float64)
            Dn = (kf * kf * Z.real).sum(axis=1, dtype=st).astype(np.float64)
            w = w64 / S2u
            c1, c2 = -TWO_PI * g, -TWO_PI * TWO_PI * Dn
            q = 2 * w * C * c1
            h = 2 * w * (c1 * c1 + C * c2)
            e = -2 * TWO_PI * TWO_PI * w * C * C * (T2u / S2u)
            chi = w64 * (PPu - C * C / S2u)
            S = np.array([q.sum(), (kap * q).sum(), h.sum(), (kap * h).sum(), (kap * kap * h).sum(),
                          e.sum(), (kap * e).sum(), (kap * kap * e).sum(), chi.sum()])
            return S, C, chi

        # ---- coarse start
        best = None
        for it in range(ndm):
            i = it - ndm // 2
            ph = p0s + kap * (i * dm_step)
            ph = ph - np.rint(ph)
            Xb = (wt[u, s].astype(st)[:, None] * (Xs * _turn(k, ph, single))).sum(axis=0) if n else np.zeros(K, X.dtype)
            Y = np.zeros(N // 2 + 1, dtype=X.dtype)
            Y[1:K + 1] = Xb
            if single:
                import scipy.fft
                Cg = scipy.fft.irfft(Y, n=N) * st(N)
            else:
                Cg = np.fft.irfft(Y, n=N) * N
            j = int(np.argmax(Cg))
            key = (-float(Cg[j]), abs(i), i)
            if best is None or key < best[0]:
                best = (key, i, j, Cg)
        _, bi, bj, Cg = best
        peak = (Cg >= np.roll(Cg, 1)) & (Cg > np.roll(Cg, -1))
        v = np.sort(Cg[peak])[::-1]
        tie[s] = v.size >= 2 and v[0] > 0 and (v[0] - v[1]) < 1e-3 * v[0]
        jw = bj - N if 2 * bj >= N else bj
        phi, d = jw / N, bi * dm_step
        nev, status = 0, 1
        if n < 2 or not kspan > 0:
            status = 2
        else:
            tphi, td, pp, pd, g0 = phi, d, 0.0, 0.0, (0.0, 0.0)
            while True:
                S = ev(tphi, td)[0]
                nev += 1
                if nev == 1 or abs(S[0] * pp + S[1] * pd) <= abs(g0[0] * pp + g0[1] * pd):
                    phi, d, g0 = tphi, td, (S[0], S[1])
                    pp, pd = _newton(S, kspan, N)
                else:
                    pp, pd = 0.5 * pp, 0.5 * pd
                if abs(pp) < TOL and abs(pd) * kspan < TOL:
                    phi, d, status = phi + pp, d + pd, 0
                    break
                if nev >= EVALS:
                    break
                tphi, td = phi + pp, d + pd
        if n:
            S, C, chi = ev(phi, d)
            prof[u, s] = np.stack([C / S2u, np.sqrt(1.0 / (w64 * S2u)), chi, np.ones(n)], axis=1)
        else:
            S = np.zeros(9)
        a11, a12, a22 = -0.5 * S[2], -0.5 * S[3], -0.5 * S[4]
        det = a11 * a22 - a12 * a12
        degen = status == 2 or not (a11 > 0 and det > 0)
        phi = phi - np.rint(phi)
        if phi >= 0.5:
            phi -= 1.0
        out[s] = (phi, np.inf if degen else np.sqrt(a22 / det), d, np.inf if degen else np.sqrt(a11 / det),
                  0.0 if degen else -a12 / det, S[8], 2.0 * K * n - n - 2.0, n, nev, 2 if degen else status)
    return out, prof, tie


def wide_ref(profs, spec, nharm, kappa, phi0, wt, ndm=1, dm_step=0.0):
    """The model: (out float64 [nsub, 10] (``COLS``), prof float64 [nchan, nsub,
    4]) of profiles [nchan, nsub, N] against the float32 table ``spec`` [1 or
    nchan, K + 1, 2]."""
    return _fit(profs, spec, nharm, kappa, phi0, wt, ndm, dm_step, False)[:2]


def wide_f32(profs, spec, nharm, kappa, phi0, wt, ndm=1, dm_step=0.0):
    """The model's steps with single-precision spectra and harmonic sums."""
    return _fit(profs, spec, nharm, kappa, phi0, wt, ndm, dm_step, True)[:2]


def near_tie(profs, spec, nharm, kappa, phi0, wt, ndm=1, dm_step=0.0):
    return _fit(profs, spec, nharm, kappa, phi0, wt, ndm, dm_step, False)[2]


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def band(nchan, turns_per_dm=40.0):
    """kappa [nchan] of a 1200 .. 1600 MHz band whose lowest channel turns by
    ``turns_per_dm`` per unit of DM (a DM of hundreds of turns across the band
    is then a DM of ten and more)."""
    f = np.linspace(1200.0, 1600.0, nchan)
    return turns_per_dm * (f[0] / f) ** 2


def dm_step_half_bin(kappa, nbin):
    """The step that moves the band edges by half a bin relative to each other."""
    return 0.5 / (nbin * (np.max(kappa) - np.min(kappa)))


def portrait(tmpl, tau, b, noise_snr, spec, rng):
    """Profiles [n, N]: b s(phi - tau) + a per row of ``tmpl`` [n or 1, N],
    with noise at b / b_err = noise_snr per profile (None: noise-free).
    Returns (profiles, sigma_F^2 [n]) -- the variance of Re and of Im of P_k."""
    n, N = len(tau), tmpl.shape[-1]
    prof = np.empty((n, N))
    s = spec.astype(np.float64)
    S2 = np.broadcast_to((s[:, 1:] ** 2).sum(axis=(1, 2)), (n,))
    snr = 1000.0 if noise_snr is None else noise_snr
    sig = (b / snr) * np.sqrt(2.0 * S2 / N)
    for i in range(n):
        prof[i] = ref.shifted(tmpl[i if tmpl.shape[0] > 1 else 0], tau[i], b[i], 0.1 * (i % 3))[0]
        if noise_snr is not None:
            prof[i] += rng.standard_normal(N) * sig[i]
    return prof, N * sig * sig / 2.0


BINS = (32, 256, 2048, 50, 97)
SNRS = (None, 10.0, 100.0, 1000.0)        # per channel, cycled over the sub-integrations; None: noise-free
NDMS = (1, 5)


def nharms(nbin):
    """A few harmonics (groups of 4 lanes), a middle value, more than there are."""
    return (4, max(9, (nbin - 1) // 4), nbin)


def shapes(nbin, nharm):
    """(nchan, nsub): three channels of one sub-integration, five of five,
    and one channel more than an evaluation block holds."""
    cb = eval_block(ref.harmonics(nbin, nharm))[1]
    return ((3, 1), (5, 5), (cb + 1, 5))


def case_inputs(nbin, nchan, nsub, per_chan, nharm, ndm, seed=0):
    """The inputs of one kernel case, a dict: ``profiles`` float32 [nchan, nsub,
    nbin], ``spec``, ``kappa``, ``phi0``, ``wt`` float32 [nchan, nsub], ``ndm``,
    ``dm_step``, and the injected ``phi`` and ``d`` [nsub].  Templates as in
    toa_ref.case_inputs.  The injected phases walk through the wrap; the
    injected d lies within a third of a bin across the band of d = 0 (ndm = 1)
    or anywhere between the outer trials (ndm > 1).  The noise level is that of
    ``SNRS[s % 4]`` in every channel of sub-integration s."""
    rng = np.random.default_rng([nbin, nchan, nsub, int(per_chan), nharm, ndm, seed, 77])
    kinds = ("multi", "inter")
    if per_chan:
        tm = np.stack([ref.make_template(nbin, kinds[c % 2]) * (1 + c / 4) for c in range(nchan)])
    else:
        tm = ref.make_template(nbin, kinds[seed % 2])[None]
    spec = ref.template_table(tm, nharm)
    kappa = band(nchan)
    step = dm_step_half_bin(kappa, nbin) if ndm > 1 else 0.0
    span = kappa.max() - kappa.min()
    edge = np.array([-0.5, 0.5 - 0.3 / nbin, 0.2 / nbin, -0.125, 0.25])
    phi = np.concatenate([edge, rng.uniform(-0.5, 0.5, max(nsub - edge.size, 0))])[:nsub]
    if ndm > 1:
        d = rng.uniform(-0.45, 0.45, nsub) * ndm * step
    else:
        d = rng.uniform(-1.0, 1.0, nsub) / (3.0 * nbin * span)
    phi0 = ref.circ(rng.uniform(-0.5, 0.5, nchan))
    prof = np.empty((nchan, nsub, nbin))
    wt = np.empty((nchan, nsub), dtype=np.float32)
    for s in range(nsub):
        b = rng.uniform(0.5, 2.0, nchan)
        p, sf2 = portrait(tm, phi0 + phi[s] + kappa * d[s], b, SNRS[s % len(SNRS)], spec, rng)
        prof[:, s] = p
        wt[:, s] = 1.0 / sf2
    return dict(profiles=prof.astype(np.float32), spec=spec, kappa=kappa, phi0=phi0, wt=wt, ndm=ndm, dm_step=step,
                phi=phi, d=d, nharm=nharm)


def model_args(c):
    return (c["profiles"], c["spec"], c["nharm"], c["kappa"], c["phi0"], c["wt"], c["ndm"], c["dm_step"])


def all_cases():
    """Every (nbin, per_chan, nharm, ndm, nchan, nsub) of the kernel's agreement test."""
    for nbin in BINS:
        for per_chan in (False, True):
            for nharm in nharms(nbin):
                for ndm in NDMS:
                    for nchan, nsub in shapes(nbin, nharm):
                        yield nbin, per_chan, nharm, ndm, nchan, nsub


def low_signal(ndraw, snr=3.0, nchan=16, nbin=256, seed=20261021):
    """The low-signal configuration: ``ndraw`` sub-integrations of ``nchan``
    channels of ``nbin`` bins, every channel at b / b_err = ``snr``, one phase
    and one d (a third of a bin across the band) for all.  A dict as
    ``case_inputs`` gives, with the per-channel phases ``tau`` [nchan]."""
    rng = np.random.default_rng(seed)
    tm = ref.make_template(nbin)[None]
    spec = ref.template_table(tm, nbin)
    kappa = band(nchan)
    phi, d = 0.1234, 1.0 / (3.0 * nbin * (kappa.max() - kappa.min()))
    phi0 = ref.circ(rng.uniform(-0.5, 0.5, nchan))
    tau = phi0 + phi + kappa * d
    prof = np.empty((nchan, ndraw, nbin))
    wt = np.empty((nchan, ndraw), dtype=np.float32)
    for s in range(ndraw):
        p, sf2 = portrait(tm, tau, np.ones(nchan), snr, spec, rng)
        prof[:, s], wt[:, s] = p, 1.0 / sf2
    return dict(profiles=prof, spec=spec, kappa=kappa, phi0=phi0, wt=wt, ndm=1, dm_step=0.0,
                phi=np.full(ndraw, phi), d=np.full(ndraw, d), nharm=nbin, tau=ref.circ(tau))
