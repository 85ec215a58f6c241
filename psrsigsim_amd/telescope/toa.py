"""Pulse arrival times from folded profiles: Taylor's (1992) Fourier-domain template match (FFTFIT) of
every (channel, sub-integration) profile of a fold-mode signal on the device, the DM the arrival times
imply, the wideband fit of one phase and one DM per sub-integration to all channels at once (Pennucci,
Demorest & Ransom 2014), and Tempo2 ``.tim`` output."""
from decimal import Decimal, getcontext

import numpy as np
import torch

from .._units import to_value
from .. import _engine, _lib
from ..utils.constants import DM_K_VALUE
from .plane import PlaneStage, _integers

MIN_BINS, MAX_BINS = 8, 8192            # the profile lengths pss_toa_fit takes
COLUMNS = ("shift", "shift_err", "scale", "scale_err", "offset", "rms", "snr", "status")
WIDE_COLUMNS = ("shift", "shift_err", "d", "dm_err", "cov", "chi2", "dof", "nchan_used", "nev", "status")


def _wrap(x):
    """Turns brought to [-1/2, 1/2)."""
    x = np.asarray(x, dtype=np.float64)
    return x - np.floor(x + 0.5)


def _tim_start(what, imjd, smjd):
    """The start of an observation for ``write_tim``: seconds of day ``imjd`` as a Decimal."""
    if int(imjd) != imjd:
        raise ValueError("%s: imjd %r is not an integer day" % (what, imjd))
    getcontext().prec = 50
    return Decimal(smjd) if isinstance(smjd, (str, Decimal, int)) else Decimal(repr(float(smjd)))


def _tim_mjd(imjd, start, t_sec):
    """The MJD of ``start`` + ``t_sec`` seconds after day ``imjd``, 16 decimals, in decimal arithmetic."""
    sec = start + Decimal(float(t_sec))                                     # (a float64 converts exactly)
    day = sec // 86400
    frac = ((sec - day * 86400) / 86400).quantize(Decimal("1e-16"))
    if frac >= 1:                                                           # (rounded up to the next day)
        day, frac = day + 1, frac - 1
    return "%d.%s" % (int(imjd) + int(day), format(frac, ".16f")[2:])


class TOATemplate(object):
    """Result of :meth:`Backend.toa_template`: the spectrum of a template
    portrait as ``pss_toa_fit`` takes it, planned on the host.

    ``spec``   float32 [ntmpl, K + 1, 2]: (Re S_k, Im S_k), k = 0 .. K, of the
               unnormalised transform S_k = sum_n s_n e^{-2 pi i k n / nbin}
               (float64 ``rfft``, rounded once; S_0 enters the offset alone)
    ``nbin``   bins of a profile
    ``K``      harmonics of the fit, min(nharm, (nbin - 1) // 2)
    ``ntmpl``  1 (one template for every channel) or the number of channels
    ``S2``     float64 [ntmpl]: sum_{k = 1 .. K} |S_k|^2 of the rounded table
    ``S0``     float64 [ntmpl]: S_0 of the rounded table"""

    def __init__(self, spec, nbin, K):
        self.spec = spec
        self.nbin = nbin
        self.K = K
        self.ntmpl = int(spec.shape[0])
        s = spec.astype(np.float64)
        self.S2 = (s[:, 1:, 0] ** 2 + s[:, 1:, 1] ** 2).sum(axis=1)
        self.S0 = s[:, 0, 0].copy()

    def __repr__(self):
        return "TOATemplate(%d bins, %d harmonics, %d template%s)" % (self.nbin, self.K, self.ntmpl,
                                                                     "" if self.ntmpl == 1 else "s")


class TOAs(object):
    """Result of :meth:`Backend.toas`: the template match of every profile, on the host.

    ``shift``, ``shift_err``  [Nchan, nsub] turns in [-1/2, 1/2): positive
                when the profile arrives later than the template
    ``scale``, ``scale_err``, ``offset``  the fitted b, its error and a of
                p = a + b s(phi - shift)
    ``rms``     the noise per bin the fit's residual implies
    ``snr``     scale / scale_err
    ``status``  int32: 0 converged, 1 iteration cap, 2 degenerate (errors +inf)
    ``freqs``   [Nchan] MHz;  ``period``, ``sublen``  seconds
    ``t_sec``   float64 [Nchan, nsub]: the sub-integration's midpoint plus
                shift x period, seconds from the start of the observation"""

    def __init__(self, fit, freqs, period, sublen):
        fit = np.asarray(fit, dtype=np.float64)
        for i, name in enumerate(COLUMNS[:-1]):
            setattr(self, name, np.ascontiguousarray(fit[..., i]))
        self.status = fit[..., 7].astype(np.int32)
        self.freqs = np.asarray(freqs, dtype=np.float64)
        self.period = float(period)
        self.sublen = float(sublen)
        mid = (np.arange(fit.shape[1], dtype=np.float64) + 0.5) * self.sublen
        self.t_sec = mid[None, :] + self.shift * self.period

    def __repr__(self):
        return "TOAs(%d channels x %d sub-integrations)" % self.shift.shape

    def delay_ms(self):
        """shift x period in milliseconds, [Nchan, nsub] (what ``signal.delay`` holds, modulo the period)."""
        return self.shift * self.period * 1e3

    def _good(self):
        return (self.status == 0) & np.isfinite(self.shift_err) & (self.shift_err > 0)

    def fit_dm(self, ref_freq=None):
        """The DM the arrival times imply: a weighted least squares of
        shift x period [s] on ``DM_K (f^-2 - f_ref^-2)`` plus a constant, over
        the entries with status 0, weights 1 / (shift_err x period)^2.
        ``ref_freq`` [MHz] (default: infinite frequency) moves the constant
        only.  A shift is known modulo one turn: the caller is responsible for
        delays that stay within half a period of the prediction across the
        band (unwrap or pre-align larger ones).  Returns ``(dm, dm_err,
        chi2r)``; ValueError with fewer than three usable entries or a single
        frequency."""
        good = self._good()
        f = np.broadcast_to(self.freqs[:, None], self.shift.shape)[good]
        if f.size < 3 or np.unique(f).size < 2:
            raise ValueError("fit_dm: needs at least three converged fits at two or more frequencies")
        x = DM_K_VALUE * (f ** -2.0 - (0.0 if ref_freq is None else float(to_value(ref_freq, 'MHz')) ** -2.0))
        y = self.shift[good] * self.period
        w = 1.0 / (self.shift_err[good] * self.period) ** 2
        x0 = (w * x).sum() / w.sum()                       # centred: the two parameters decouple
        xc = x - x0
        sxx = (w * xc * xc).sum()
        dm = (w * xc * y).sum() / sxx
        c = (w * y).sum() / w.sum()
        res = y - c - dm * xc
        chi2r = float((w * res * res).sum() / (f.size - 2))
        return float(dm), float(1.0 / np.sqrt(sxx)), chi2r

    def write_tim(self, path, imjd, smjd, site="@", name=None):
        """Write the converged fits as a Tempo2 ``FORMAT 1`` file: one line
        ``name freq_MHz MJD err_us site`` each, channels in order, then
        sub-integrations.  The observation starts at day ``imjd`` (an integer)
        plus ``smjd`` seconds (a number, a Decimal or a string of digits).  The
        MJD is the integer day plus the seconds in decimal arithmetic, written
        with 16 decimals (1e-16 day = 8.64 ps): no digit of ``t_sec`` below a
        nanosecond is lost to a float64 day.  Returns the number of lines."""
        start = _tim_start("write_tim", imjd, smjd)
        name = "toa" if name is None else str(name)
        good = self._good()
        lines = ["FORMAT 1"]
        for c in range(self.shift.shape[0]):
            for s in range(self.shift.shape[1]):
                if not good[c, s]:
                    continue
                mjd = _tim_mjd(imjd, start, self.t_sec[c, s])
                lines.append("%s %.6f %s %.6f %s" % (name, self.freqs[c], mjd,
                                                     self.shift_err[c, s] * self.period * 1e6, site))
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        return len(lines) - 1


class WidebandTOAs(object):
    """Result of :meth:`Backend.wideband_toas`: one phase and one DM per
    sub-integration, on the host.  [nsub] unless noted.

    ``shift``, ``shift_err``  turns in [-1/2, 1/2) at infinite frequency,
                positive when the pulse arrives later than the template
    ``dm``, ``dm_err``  the nominal DM plus the fitted offset, and its error
    ``cov``     the covariance of ``shift`` and ``dm``
    ``chi2``, ``dof``, ``chi2r``  of the fit with the weights it was given
    ``nchan_used``, ``nev``, ``status``  channels that entered, evaluations,
                int32 0 converged, 1 iteration cap, 2 degenerate (errors +inf)
    ``scale``, ``scale_err``, ``used``  [Nchan, nsub]: the amplitude of every
                channel, its error, and whether the channel entered the fit
    ``freqs``   [Nchan] MHz;  ``period``, ``sublen``  seconds
    ``ref_freq``  MHz: where phase and DM decorrelate, kappa_0 = -cov /
                dm_err^2 turns per unit of DM, nu_0 = sqrt(DM_K / (P kappa_0))
    ``shift_ref``, ``shift_ref_err``  the phase there relative to the
                prediction at the nominal DM, shift + kappa_0 (dm - nominal),
                with the variance shift_err^2 - cov^2 / dm_err^2
    ``t_sec``   the sub-integration's midpoint plus period x wrap(frac(kappa_0
                x nominal DM) + shift_ref): the arrival time at ``ref_freq``,
                seconds from the start of the observation"""

    def __init__(self, out, prof, freqs, period, sublen, dm_nominal=0.0):
        out = np.asarray(out, dtype=np.float64)
        prof = np.asarray(prof, dtype=np.float64)
        self.dm_nominal = float(dm_nominal)
        self.shift, self.shift_err = out[:, 0].copy(), out[:, 1].copy()
        d = out[:, 2]
        self.dm, self.dm_err, self.cov = self.dm_nominal + d, out[:, 3].copy(), out[:, 4].copy()
        self.chi2, self.dof = out[:, 5].copy(), out[:, 6].copy()
        with np.errstate(all="ignore"):
            self.chi2r = np.where(self.dof > 0, self.chi2 / self.dof, np.nan)
        self.nchan_used = out[:, 7].astype(np.int32)
        self.nev = out[:, 8].astype(np.int32)
        self.status = out[:, 9].astype(np.int32)
        self.scale, self.scale_err = prof[..., 0].copy(), prof[..., 1].copy()
        self.used = prof[..., 3] != 0
        self.freqs = np.asarray(freqs, dtype=np.float64)
        self.period = float(period)
        self.sublen = float(sublen)
        good = self._good()
        with np.errstate(all="ignore"):
            k0 = np.where(good, -self.cov / self.dm_err ** 2, np.nan)
            self.kappa_ref = k0
            self.ref_freq = np.where(k0 > 0, np.sqrt(DM_K_VALUE / (self.period * k0)), np.nan)
            self.shift_ref = _wrap(self.shift + k0 * d)
            self.shift_ref_err = np.sqrt(self.shift_err ** 2 - self.cov ** 2 / self.dm_err ** 2)
            mid = (np.arange(out.shape[0], dtype=np.float64) + 0.5) * self.sublen
            self.t_sec = mid + self.period * _wrap(k0 * self.dm_nominal - np.rint(k0 * self.dm_nominal) + self.shift_ref)

    def __repr__(self):
        return "WidebandTOAs(%d sub-integrations of %d channels)" % (self.shift.shape[0], self.freqs.shape[0])

    def _good(self):
        return (self.status == 0) & np.isfinite(self.shift_err) & np.isfinite(self.dm_err) & (self.dm_err > 0)

    def write_tim(self, path, imjd, smjd, site="@", name=None):
        """Write the converged sub-integrations as a Tempo2 ``FORMAT 1`` file:
        one line ``name ref_freq_MHz MJD err_us site -pp_dm DM -pp_dme DM_err``
        each (the wideband flags of NANOGrav's data sets), the error
        ``shift_ref_err`` x period.  ``imjd``, ``smjd`` and the MJD arithmetic
        are those of :meth:`TOAs.write_tim`.  Returns the number of lines."""
        start = _tim_start("write_tim", imjd, smjd)
        name = "toa" if name is None else str(name)
        good = self._good() & np.isfinite(self.ref_freq)
        lines = ["FORMAT 1"]
        for s in np.flatnonzero(good):
            lines.append("%s %.6f %s %.6f %s -pp_dm %.10f -pp_dme %.10f"
                         % (name, self.ref_freq[s], _tim_mjd(imjd, start, self.t_sec[s]),
                            self.shift_ref_err[s] * self.period * 1e6, site, self.dm[s], self.dm_err[s]))
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        return len(lines) - 1


def wideband_plan(freqs_MHz, period, dm):
    """(kappa, phi0) float64 [Nchan] of ``pss_toa_wide_fit``: kappa = DM_K
    nu^-2 / P turns per unit of DM, phi0 = kappa x dm reduced to [-1/2, 1/2)."""
    f = np.asarray(freqs_MHz, dtype=np.float64)
    kappa = DM_K_VALUE * f ** -2.0 / float(period)
    return kappa, _wrap(kappa * float(dm))


class TOAStage(PlaneStage):
    @staticmethod
    def toa_template(source, nbin, Nchan=None, nharm=None):
        """The template of :meth:`fit_profiles` and :meth:`toas`, planned on
        the host.  ``source`` is a ``Pulsar`` (its portrait), a portrait (its
        ``calc_profiles`` at the phases n / nbin; ``Nchan`` channels) or an
        array [nbin] / [Nchan, nbin].  The float64 ``rfft`` of every row is
        rounded once to float32; rows that are all alike give one template.
        ``nharm`` (default: all) limits the harmonics to K = min(nharm,
        (nbin - 1) // 2); the Nyquist harmonic is never used.  ValueError for
        a template row without power in those harmonics.  Returns a
        :class:`TOATemplate`."""
        what = "toa_template"
        (nb,) = _integers(what, "nbin", nbin)
        if not (MIN_BINS <= nb <= MAX_BINS):
            raise ValueError("%s: nbin %d outside [%d, %d]" % (what, nb, MIN_BINS, MAX_BINS))
        kmax = (nb - 1) // 2
        if nharm is None:
            K = kmax
        else:
            (nh,) = _integers(what, "nharm", nharm)
            if nh < 1:
                raise ValueError("%s: nharm %d < 1" % (what, nh))
            K = min(nh, kmax)
        portrait = getattr(source, "Profiles", source)
        if hasattr(portrait, "calc_profiles"):
            prof = portrait.calc_profiles(np.arange(nb) / nb, Nchan=Nchan)
        else:
            prof = portrait
        prof = np.asarray(prof, dtype=np.float64)
        if prof.ndim == 1:
            prof = prof[None]
        if prof.ndim != 2 or prof.shape[1] != nb:
            raise ValueError("%s: the template has the shape %s for %d bins" % (what, prof.shape, nb))
        if Nchan is not None and prof.shape[0] not in (1, int(Nchan)):
            raise ValueError("%s: %d template rows for %d channels" % (what, prof.shape[0], int(Nchan)))
        if not np.isfinite(prof).all():
            raise ValueError("%s: the template is not finite" % what)
        if prof.shape[0] > 1 and (prof.strides[0] == 0 or (prof == prof[0]).all()):
            prof = prof[:1]
        S = np.fft.rfft(prof, axis=1)[:, :K + 1]
        spec = np.ascontiguousarray(np.stack([S.real, S.imag], axis=-1).astype(np.float32))
        t = TOATemplate(spec, nb, K)
        if not (t.S2 > 0).all():
            raise ValueError("%s: template row %d has no power in the harmonics 1 .. %d"
                             % (what, int(np.flatnonzero(~(t.S2 > 0))[0]), K))
        return t

    @staticmethod
    def fit_profiles(data, nchan, nsub, nbin, template):
        """FFTFIT of the nchan x nsub profiles of ``data`` on the device
        (``pss_toa_fit``, include/pss_hip.h): ``data`` is a float32 device
        tensor of at least ``nchan`` rows, profile (c, s) at data[c, s * nbin :
        (s + 1) * nbin] -- a fold-mode signal's own layout, nothing is copied.
        Returns the float32 device tensor [nchan, nsub, 8]: tau, tau_err, b,
        b_err, a, rms, snr, status.  No host synchronisation."""
        what = "fit_profiles"
        nc, ns, nb = _integers(what, "nchan, nsub and nbin", nchan, nsub, nbin)
        if not isinstance(template, TOATemplate):
            raise ValueError("%s: template must be a TOATemplate (Backend.toa_template)" % what)
        if template.nbin != nb:
            raise ValueError("%s: the template has %d bins, the profiles %d" % (what, template.nbin, nb))
        if template.ntmpl not in (1, nc):
            raise ValueError("%s: %d templates for %d channels" % (what, template.ntmpl, nc))
        if not isinstance(data, torch.Tensor) or data.dim() != 2 or int(data.shape[0]) < nc \
                or int(data.shape[1]) < ns * nb or nc < 1 or ns < 1:
            raise ValueError("%s takes a device tensor of at least %d rows of %d x %d samples" % (what, nc, ns, nb))
        data, ld = PlaneStage._plane_rows(data)
        spec_d = _engine.to_dev(template.spec)
        out = torch.empty((nc, ns, 8), dtype=torch.float32, device=data.device)
        rc = _lib.lib().pss_toa_fit(_engine.ptr(data), nc, ns, nb, ld, _engine.ptr(spec_d), template.ntmpl,
                                    template.K, _engine.ptr(out), 8, _engine.stream_ptr())
        _lib.check(rc, "toa_fit")
        return out

    @staticmethod
    def fit_wideband(data, nchan, nsub, nbin, template, kappa, phi0, wt, ndm=1, dm_step=0.0):
        """The wideband fit of ``pss_toa_wide_fit`` (include/pss_hip.h) on the
        device: one phase and one DM offset per sub-integration from all
        ``nchan`` profiles of it.  ``data``, ``nchan``, ``nsub``, ``nbin`` and
        ``template`` as in :meth:`fit_profiles`; ``kappa`` and ``phi0`` [nchan]
        (float64: turns per unit of DM, and the phase predicted at the nominal
        DM in [-1/2, 1/2)); ``wt`` [nchan, nsub] (float32: the inverse variance
        of Re and of Im of a harmonic; <= 0 or non-finite leaves a profile
        out); ``ndm`` (odd) trials ``dm_step`` apart start the iteration.
        Arrays or device tensors.  The workspace comes from torch's caching
        allocator, per call.  Returns the device tensors (float64 [nsub, 10]:
        phi, phi_err, d, d_err, cov, chi2, dof, channels used, evaluations,
        status; float32 [nchan, nsub, 4]: b, b_err, the chi2 term, used).  No
        host synchronisation."""
        what = "fit_wideband"
        nc, ns, nb = _integers(what, "nchan, nsub and nbin", nchan, nsub, nbin)
        (nd,) = _integers(what, "ndm", ndm)
        if not isinstance(template, TOATemplate):
            raise ValueError("%s: template must be a TOATemplate (Backend.toa_template)" % what)
        if template.nbin != nb:
            raise ValueError("%s: the template has %d bins, the profiles %d" % (what, template.nbin, nb))
        if template.ntmpl not in (1, nc):
            raise ValueError("%s: %d templates for %d channels" % (what, template.ntmpl, nc))
        if not isinstance(data, torch.Tensor) or data.dim() != 2 or int(data.shape[0]) < nc \
                or int(data.shape[1]) < ns * nb or nc < 1 or ns < 1:
            raise ValueError("%s takes a device tensor of at least %d rows of %d x %d samples" % (what, nc, ns, nb))
        if nd < 1 or nd % 2 == 0:
            raise ValueError("%s: ndm %d is not odd and >= 1" % (what, nd))
        step = float(dm_step)
        if not (np.isfinite(step) and step >= 0):
            raise ValueError("%s: dm_step %r is not finite and >= 0" % (what, dm_step))

        tables = (("kappa", kappa, (nc,), torch.float64, np.float64), ("phi0", phi0, (nc,), torch.float64, np.float64),
                  ("wt", wt, (nc, ns), torch.float32, np.float32))
        for name, v, shape, _, _ in tables:
            have = tuple(v.shape) if isinstance(v, torch.Tensor) else np.shape(v)
            if have != shape:
                raise ValueError("%s: %s has the shape %s, not %s" % (what, name, have, shape))
        kap, ph0, wts = (v.to(device=data.device, dtype=td).contiguous() if isinstance(v, torch.Tensor)
                         else _engine.to_dev(np.ascontiguousarray(np.asarray(v, dtype=nd_)))
                         for _, v, _, td, nd_ in tables)
        data, ld = PlaneStage._plane_rows(data)
        spec_d = _engine.to_dev(template.spec)
        L = _lib.lib()
        nbytes = int(L.pss_toa_wide_workspace_bytes(nc, ns, nb, template.K, nd))
        work = torch.empty((nbytes,), dtype=torch.uint8, device=data.device)
        out = torch.empty((ns, 10), dtype=torch.float64, device=data.device)
        prof = torch.empty((nc, ns, 4), dtype=torch.float32, device=data.device)
        rc = L.pss_toa_wide_fit(_engine.ptr(data), nc, ns, nb, ld, _engine.ptr(spec_d), template.ntmpl, template.K,
                                _engine.ptr(kap), _engine.ptr(ph0), _engine.ptr(wts), nd, step, _engine.ptr(out), 10,
                                _engine.ptr(prof), 4, _engine.ptr(work), nbytes, _engine.stream_ptr())
        _lib.check(rc, "toa_wide_fit")
        return out, prof

    def wideband_toas(self, signal, pulsar=None, template=None, nharm=None, dm=None, weights=None, ndm=1,
                      dm_step=None):
        """Wideband arrival times of a fold-mode ``FilterBankSignal``: one
        phase and one DM per sub-integration, fitted to all its channels at
        once (:meth:`fit_wideband`), where :meth:`toas` fits every profile on
        its own -- which it can only while every channel has the signal to be
        fitted alone.  ``dm`` is the DM still present in the folded profiles
        (default: ``signal.dm``, or 0); kappa and phi0 are planned from it on
        the host in float64, from the signal's frequencies and the fold period.
        ``weights`` [Nchan, nsub] are the inverse variances of a harmonic's
        real part; by default one :meth:`fit_profiles` pass supplies every
        profile's ``rms`` and the weight is 2 / (nbin rms^2) where that is
        finite and > 0, else 0 -- an extra pass over the data, the price of not
        being told the noise.  ``ndm`` (odd) trials start the iteration,
        ``dm_step`` apart (default: the step that moves the band's edges by
        half a bin relative to each other).  ValueError for a search-mode
        signal, a row ``nsub`` does not divide, and a signal that holds a shard
        of the band (the fit needs every channel).  Returns
        :class:`WidebandTOAs` (one host synchronisation)."""
        what = "wideband_toas"
        if not getattr(signal, "fold", False):
            raise ValueError("%s takes a fold-mode signal (FilterBankSignal(fold=True))" % what)
        data = signal.data
        nsub = int(signal.nsub)
        ncols = int(data.shape[1])
        if nsub < 1 or ncols % nsub:
            raise ValueError("%s: %d sub-integrations do not divide a row of %d samples" % (what, nsub, ncols))
        nbin = ncols // nsub
        nchan = int(data.shape[0])
        c0, c1 = signal.shard
        if (c0, c1) != (0, int(signal.Nchan)):
            raise ValueError("%s: the signal holds the channels %d .. %d of %d; a wideband fit needs every channel"
                             % (what, c0, c1, int(signal.Nchan)))
        if template is None:
            if pulsar is None:
                raise ValueError("%s needs a pulsar or a template" % what)
            template = self.toa_template(pulsar, nbin, Nchan=signal.Nchan, nharm=nharm)
        (nd,) = _integers(what, "ndm", ndm)
        if nd < 1 or nd % 2 == 0:
            raise ValueError("%s: ndm %d is not odd and >= 1" % (what, nd))
        if dm is None:
            dm = signal.dm
        dm = 0.0 if dm is None else float(to_value(dm, 'pc/cm^3'))
        period = nbin / (signal._samprate_MHz() * 1e6)
        freqs = signal._freqs_MHz()
        kappa, phi0 = wideband_plan(freqs, period, dm)
        if dm_step is None:
            span = float(kappa.max() - kappa.min())
            dm_step = 0.5 / (nbin * span) if nd > 1 and span > 0 else 0.0
        if weights is None:
            rms = self.fit_profiles(data, nchan, nsub, nbin, template)[:, :, 5]
            wt = 2.0 / (nbin * rms * rms)
            wt = torch.where(torch.isfinite(wt) & torch.isfinite(rms) & (rms > 0), wt, torch.zeros_like(wt))
        else:
            wt = weights
        out, prof = self.fit_wideband(data, nchan, nsub, nbin, template, kappa, phi0, wt, nd, dm_step)
        return WidebandTOAs(out.cpu().numpy(), prof.cpu().numpy(), freqs, period,
                            float(to_value(signal.sublen, 's')), dm)

    def toas(self, signal, pulsar=None, template=None, nharm=None):
        """Arrival times of a fold-mode ``FilterBankSignal`` (extension: the
        reference writes its folded profiles to PSRFITS for an outside tool):
        every (channel, sub-integration) profile is matched against
        ``template`` (a :class:`TOATemplate`; default: ``pulsar``'s own
        portrait at the signal's channels and bins, :meth:`toa_template`).
        The signal's row holds ``nsub`` profiles of nbin = row length / nsub
        bins; ValueError for a search-mode signal and for a row that ``nsub``
        does not divide.  The period of the result is that of the fold, nbin /
        sample rate.  Returns :class:`TOAs` (one host synchronisation)."""
        what = "toas"
        if not getattr(signal, "fold", False):
            raise ValueError("%s takes a fold-mode signal (FilterBankSignal(fold=True))" % what)
        data = signal.data
        nsub = int(signal.nsub)
        ncols = int(data.shape[1])
        if nsub < 1 or ncols % nsub:
            raise ValueError("%s: %d sub-integrations do not divide a row of %d samples" % (what, nsub, ncols))
        nbin = ncols // nsub
        nchan = int(data.shape[0])
        c0, c1 = signal.shard
        if template is None:
            if pulsar is None:
                raise ValueError("%s needs a pulsar or a template" % what)
            template = self.toa_template(pulsar, nbin, Nchan=signal.Nchan, nharm=nharm)
        if template.ntmpl not in (1, nchan) and template.ntmpl == signal.Nchan:
            template = TOATemplate(np.ascontiguousarray(template.spec[c0:c1]), template.nbin, template.K)
        fit = self.fit_profiles(data, nchan, nsub, nbin, template).cpu().numpy()
        period = nbin / (signal._samprate_MHz() * 1e6)
        return TOAs(fit, signal._freqs_MHz()[c0:c1], period, float(to_value(signal.sublen, 's')))
