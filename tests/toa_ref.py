"""The float64 model of the template match ``pss_toa_fit`` (include/pss_hip.h),
its single-precision restatement, and the inputs the TOA tests share.

* ``fftfit_ref``   -- the model: NumPy ``rfft`` in float64, the coarse maximum
  on the grid j / N, the root of C' by bisection to convergence.  It fixes every
  corner the header describes (wrap, K = 1, degenerate and non-finite profiles);
  the kernel follows it.
* ``fftfit_f32``   -- the same steps with every array in float32 and SciPy's
  single-precision pocketfft: what float32 arithmetic alone costs.  The GPU
  tests take their tolerance from its distance to the model.
* ``near_tie``     -- whether the model's two highest local maxima of the
  coarse correlation lie within 1e-3 of the maximum of each other.
* ``template_table``, ``make_template``, ``shifted`` -- inputs.
"""
import numpy as np

COLS = ("tau", "tau_err", "b", "b_err", "a", "rms", "snr", "status")
TWO_PI = 2.0 * np.pi


def harmonics(nbin, nharm):
    return min(int(nharm), (int(nbin) - 1) // 2)


def template_table(tmpl, nharm):
    """float32 [..., K + 1, 2] of template profiles [..., N] (float64 rfft, rounded once)."""
    t = np.asarray(tmpl, dtype=np.float64)
    K = harmonics(t.shape[-1], nharm)
    S = np.fft.rfft(t, axis=-1)[..., :K + 1]
    return np.stack([S.real, S.imag], axis=-1).astype(np.float32)


def _fit(profs, spec, nharm, dt):
    single = dt == np.float32
    ct = np.complex64 if single else np.complex128
    p = np.atleast_2d(np.asarray(profs)).astype(dt)
    n, N = p.shape
    K = harmonics(N, nharm)
    spec = np.asarray(spec, dtype=np.float32)
    assert spec.shape[-2:] == (K + 1, 2)
    S = (spec[..., 0].astype(dt) + 1j * spec[..., 1].astype(dt)).astype(ct)
    S = np.broadcast_to(S, (n, K + 1))
    finite = np.isfinite(p).all(axis=1)
    # the first sample is taken off before the transform and given back to P_0:
    # the harmonics k >= 1 do not see it, and a constant profile is exact zeros
    # whatever the transform does at that length
    p0 = np.where(finite, p[:, 0], dt(0))
    pz = np.where(finite[:, None], p - p0[:, None], dt(0))
    if single:
        import scipy.fft
        P = scipy.fft.rfft(pz, axis=1)
        assert P.dtype == np.complex64
    else:
        P = np.fft.rfft(pz, axis=1)
    P0, Pk, Sk, S0 = P[:, 0].real + dt(N) * p0, P[:, 1:K + 1], S[:, 1:], S[:, 0].real
    X = Pk * np.conj(Sk)
    S2 = (Sk.real * Sk.real + Sk.imag * Sk.imag).sum(axis=1, dtype=dt)
    PP = (Pk.real * Pk.real + Pk.imag * Pk.imag).sum(axis=1, dtype=dt)
    Y = np.zeros((n, N // 2 + 1), dtype=ct)
    Y[:, 1:K + 1] = X
    if single:
        Cg = scipy.fft.irfft(Y, n=N, axis=1)
    else:
        Cg = np.fft.irfft(Y, n=N, axis=1)
    jstar = np.argmax(Cg, axis=1)                              # the first maximum
    k = np.arange(1, K + 1, dtype=np.int64)
    base = (((k[None, :] * jstar[:, None]) % N).astype(dt) / dt(N))
    kf = k.astype(dt)

    def ev(delta):
        r = base + kf[None, :] * delta[:, None]
        r = r - np.rint(r)
        ang = dt(TWO_PI) * r
        Z = X * (np.cos(ang) + 1j * np.sin(ang)).astype(ct)
        return (Z.real.sum(axis=1, dtype=dt), (kf * Z.imag).sum(axis=1, dtype=dt),
                (kf * kf * Z.real).sum(axis=1, dtype=dt))

    lo = np.full(n, -1.0 / N, dtype=dt)
    hi = np.full(n, 1.0 / N, dtype=dt)
    for _ in range(30 if single else 70):
        mid = dt(0.5) * (lo + hi)
        g = ev(mid)[1]
        up = g < 0                                             # C' = -2 pi g > 0: the maximum lies above
        lo = np.where(up, mid, lo)
        hi = np.where(up, hi, mid)
    delta = dt(0.5) * (lo + hi)
    C, _, D = ev(delta)
    degen = ~(C > 0) | ~(D > 0)
    jw = np.where(2 * jstar >= N, jstar - N, jstar)
    with np.errstate(all="ignore"):
        tau = jw.astype(dt) / dt(N) + np.where(degen, dt(0), delta)
        tau = np.where(tau >= 0.5, tau - 1, tau)
        tau = np.where(tau < -0.5, tau + 1, tau)
        b = C / S2
        a = (P0 - b * S0) / dt(N)
        R = PP - C * C / S2
        sig2 = np.maximum(R, 0) / dt(2 * K - 2) if K > 1 else np.full(n, np.inf, dtype=dt)
        tau_err = np.where(degen, np.inf, np.sqrt(sig2 / (b * D)) / dt(TWO_PI))
        b_err = np.where(degen, np.inf, np.sqrt(sig2 / S2))
        rms = np.sqrt(dt(2) * sig2 / dt(N))
        snr = b / b_err
        # the squares of the three noise figures before R is clamped at 0
        s2u = R / dt(2 * K - 2) if K > 1 else sig2
        sq = np.stack([np.where(degen, np.inf, s2u / (b * D) / dt(TWO_PI) ** 2), np.where(degen, np.inf, s2u / S2),
                       dt(2) * s2u / dt(N)], axis=1).astype(np.float64)
    out = np.stack([tau, tau_err, b, b_err, a, rms, snr, np.where(degen, 2.0, 0.0)], axis=1).astype(np.float64)
    bad = ~finite
    out[bad] = (0.0, np.inf, np.nan, np.inf, np.nan, np.nan, np.nan, 2.0)
    sq[bad] = (np.inf, np.inf, np.nan)
    return out, Cg, sq


def fftfit_ref(profs, spec, nharm):
    """The model: float64 [n, 8] (``COLS``) of profiles [n, N] (or one [N])
    against the float32 table ``spec`` [K + 1, 2] or [n, K + 1, 2]."""
    return _fit(profs, spec, nharm, np.float64)[0]


def fftfit_f32(profs, spec, nharm):
    """The model's steps in float32 (SciPy's single-precision transform)."""
    return _fit(profs, spec, nharm, np.float32)[0]


def noise_squares(profs, spec, nharm, dtype=np.float64):
    """float64 [n, 3]: tau_err^2, b_err^2 and rms^2 as the model (or, with
    float32, its restatement) has them before the residual R is clamped at 0.
    On a noise-free profile R is a rounding residue of either sign: the clamp
    would hide what the arithmetic cost."""
    return _fit(profs, spec, nharm, dtype)[2]


def near_tie(profs, spec, nharm, frac=1e-3):
    """bool [n]: the model's two highest local maxima of C on the grid differ
    by less than ``frac`` of the maximum."""
    Cg = _fit(profs, spec, nharm, np.float64)[1]
    peak = (Cg >= np.roll(Cg, 1, axis=1)) & (Cg > np.roll(Cg, -1, axis=1))
    out = np.zeros(len(Cg), dtype=bool)
    for i, (c, m) in enumerate(zip(Cg, peak)):
        v = np.sort(c[m])[::-1]
        out[i] = v.size >= 2 and v[0] > 0 and (v[0] - v[1]) < frac * v[0]
    return out


def circ(d):
    """A difference of turns brought to [-1/2, 1/2)."""
    d = np.asarray(d, dtype=np.float64)
    return d - np.floor(d + 0.5)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def make_template(nbin, kind="multi"):
    """A template of ``nbin`` bins, float64, sampled from von Mises components
    (smooth and periodic at any nbin): ``multi`` a main pulse with two
    shoulders; ``inter`` a main pulse and an interpulse at 0.9 of its height
    half a turn away."""
    ph = np.arange(nbin) / nbin

    def vm(c, w, a):
        kappa = 1.0 / (TWO_PI * w) ** 2
        return a * np.exp(kappa * (np.cos(TWO_PI * (ph - c)) - 1.0))

    if kind == "multi":
        return vm(0.30, 0.03, 1.0) + vm(0.36, 0.05, 0.45) + vm(0.22, 0.08, 0.2) + 0.1
    if kind == "inter":
        return vm(0.25, 0.04, 1.0) + vm(0.75, 0.04, 0.9) + 0.05
    raise ValueError(kind)


def shifted(tmpl, tau, b=1.0, a=0.0):
    """a + b s(phi - tau) by the Fourier shift theorem, float64.  An even
    length's Nyquist term is shifted as a cosine (it never enters a fit)."""
    t = np.asarray(tmpl, dtype=np.float64)
    N = t.shape[-1]
    S = np.fft.rfft(t)
    k = np.arange(S.size)
    tau = np.atleast_1d(np.asarray(tau, dtype=np.float64))
    Z = S[None, :] * np.exp(-1j * TWO_PI * k[None, :] * tau[:, None])
    if N % 2 == 0:
        Z[:, -1] = (S[-1] * np.cos(TWO_PI * k[-1] * tau)).real
    col = lambda v: np.asarray(v, dtype=np.float64).reshape(-1, 1)      # noqa: E731
    return col(a) + col(b) * np.fft.irfft(Z, n=N, axis=1)


FFT_BINS = (32, 64, 256, 2048, 4096)
DIRECT_BINS = (8, 16, 50, 97, 1000, 8192)
SNRS = (None, 10.0, 100.0, 1000.0)        # None: noise-free


def wg_profiles(nbin):
    """Profiles a workgroup of pss_toa_fit owns at ``nbin`` bins."""
    if nbin in (32, 64, 128, 256, 512, 1024, 2048, 4096):
        return max(2, 8192 // nbin)
    return 1


def shapes(nbin):
    """(nchan, nsub) of the kernel tests: one profile a channel, several, one
    channel, and one profile more than a workgroup's."""
    return ((3, 1), (3, 5), (1, 7), (1, wg_profiles(nbin) + 1))


def nharms(nbin):
    """One harmonic, a middle value, more than there are."""
    return (1, max(2, (nbin - 1) // 4), nbin)


def band_limited(tmpl, nharm):
    """(the template rebuilt in float64 from its rounded table, the table):
    profiles shifted from it are exactly a + b s(phi - tau) for the table."""
    spec = template_table(tmpl, nharm)
    N = np.shape(tmpl)[-1]
    Y = np.zeros(spec.shape[:-2] + (N // 2 + 1,), dtype=np.complex128)
    Y[..., :spec.shape[-2]] = spec[..., 0].astype(np.float64) + 1j * spec[..., 1].astype(np.float64)
    return np.fft.irfft(Y, n=N, axis=-1), spec


def case_inputs(nbin, nchan, nsub, per_chan, nharm, seed=0):
    """The inputs of one kernel case: ``profiles`` float32 [nchan, nsub, nbin],
    the table ``spec`` float32 [ntmpl, K + 1, 2] and the injected ``tau``.
    Channel c's template is ``multi`` (even c) or ``inter`` (odd c, the
    interpulse at 0.9 of the main pulse) scaled by 1 + c / 4 when ``per_chan``,
    else ``multi`` for all -- ``inter`` for all at seed 1.  The shifts walk
    through the wrap (-1/2, within 1/nbin of +-1/2 and of 0) and then a fixed
    random set; the noise cycles through ``SNRS`` (b / b_err of the fit)."""
    rng = np.random.default_rng([nbin, nchan, nsub, int(per_chan), nharm, seed])
    kinds = ("multi", "inter")
    if per_chan:
        tm = np.stack([make_template(nbin, kinds[c % 2]) * (1 + c / 4) for c in range(nchan)])
    else:
        tm = make_template(nbin, kinds[seed % 2])[None]
    spec = template_table(tm, nharm)
    K = spec.shape[1] - 1
    n = nchan * nsub
    edge = np.array([-0.5, -0.5 + 0.3 / nbin, 0.5 - 0.3 / nbin, 0.0, 0.2 / nbin, -0.2 / nbin, 0.25, -0.125])
    tau = np.concatenate([edge, rng.uniform(-0.5, 0.5, max(n - edge.size, 0))])[:n]
    b = rng.uniform(0.5, 2.0, n)
    a = rng.uniform(-1.0, 1.0, n)
    prof = np.empty((n, nbin))
    for i in range(n):
        t = tm[(i // nsub) if per_chan else 0]
        s = spec[(i // nsub) if per_chan else 0].astype(np.float64)
        S2 = (s[1:] ** 2).sum()
        prof[i] = shifted(t, tau[i], b[i], a[i])[0]
        snr = SNRS[i % len(SNRS)]
        if snr is not None:
            prof[i] += rng.standard_normal(nbin) * (b[i] / snr) * np.sqrt(2.0 * S2 / nbin)
    return prof.astype(np.float32).reshape(nchan, nsub, nbin), spec, tau.reshape(nchan, nsub)


def per_profile(spec, nsub):
    """The table of every profile of a case: [K + 1, 2] (one template) or [nchan * nsub, K + 1, 2]."""
    return spec[0] if spec.shape[0] == 1 else np.repeat(spec, nsub, axis=0)
