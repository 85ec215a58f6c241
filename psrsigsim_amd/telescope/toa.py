"""Pulse arrival times from folded profiles: Taylor's (1992) Fourier-domain template match (FFTFIT) of
every (channel, sub-integration) profile of a fold-mode signal on the device, the DM the arrival times
imply, and Tempo2 ``.tim`` output."""
from decimal import Decimal, getcontext

import numpy as np
import torch

from .._units import to_value
from .. import _engine, _lib
from ..utils.constants import DM_K_VALUE
from .plane import PlaneStage, _integers

MIN_BINS, MAX_BINS = 8, 8192            # the profile lengths pss_toa_fit takes
COLUMNS = ("shift", "shift_err", "scale", "scale_err", "offset", "rms", "snr", "status")


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
        if int(imjd) != imjd:
            raise ValueError("write_tim: imjd %r is not an integer day" % (imjd,))
        getcontext().prec = 50
        start = Decimal(smjd) if isinstance(smjd, (str, Decimal, int)) else Decimal(repr(float(smjd)))
        name = "toa" if name is None else str(name)
        good = self._good()
        lines = ["FORMAT 1"]
        for c in range(self.shift.shape[0]):
            for s in range(self.shift.shape[1]):
                if not good[c, s]:
                    continue
                sec = start + Decimal(float(self.t_sec[c, s]))             # (a float64 converts exactly)
                day = sec // 86400
                frac = ((sec - day * 86400) / 86400).quantize(Decimal("1e-16"))
                if frac >= 1:                                               # (rounded up to the next day)
                    day, frac = day + 1, frac - 1
                mjd = "%d.%s" % (int(imjd) + int(day), format(frac, ".16f")[2:])
                lines.append("%s %.6f %s %.6f %s" % (name, self.freqs[c], mjd,
                                                     self.shift_err[c, s] * self.period * 1e6, site))
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")
        return len(lines) - 1


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
