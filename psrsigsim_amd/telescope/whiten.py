"""Spectrum whitening: block medians of the power (the noise spectrum), every bin divided by the local
median, known interference lines replaced by a neutral value (red noise, birdie zapping)."""
import numpy as np
import torch

from .._units import to_value
from .. import _engine, _lib
from .plane import PlaneStage, _integers

MAX_BLOCK = 256                          # the widest block pss_spectrum_medians selects from


class WhitenPlan(object):
    """Result of :meth:`Backend.whiten_plan`: the blocks of a spectrum of
    ``nbin`` bins over which the power's median is taken, on the host.

    ``edges``   int64 [nblk + 1], strictly increasing from ``kstart`` to
                ``nbin``; block b holds the bins edges[b] .. edges[b + 1] - 1
    ``nbin``    bins of the spectrum (the Nyquist bin left out)
    ``kstart``  the first bin of block 0; the bins below it are zeroed
    ``w0``      the narrowest planned block
    ``wmax``    the widest planned block (the last may reach 2 wmax - 1)
    ``nblk``    blocks"""

    def __init__(self, edges, nbin, kstart, w0, wmax):
        self.edges = edges
        self.nbin = nbin
        self.kstart = kstart
        self.w0 = w0
        self.wmax = wmax
        self.nblk = int(len(edges)) - 1

    def __repr__(self):
        return "WhitenPlan(%d blocks over bins %d .. %d, widths %d .. %d)" % (
            self.nblk, self.kstart, self.nbin, self.w0, self.wmax)


def _check_edges(what, edges, nbin):
    """The table of a plan as int64 [nblk + 1]; ValueError unless it is what ``pss_spectrum_medians`` takes."""
    e = np.asarray(edges)
    if e.ndim != 1 or e.size < 2 or e.dtype.kind not in "iu":
        raise ValueError("%s: the plan's edges must be a 1-D integer table of at least 2 entries" % what)
    e = np.ascontiguousarray(e, dtype=np.int64)
    w = np.diff(e)
    if e[0] < 0 or e[-1] != nbin or w.min() < 1 or w.max() > MAX_BLOCK:
        raise ValueError("%s: the plan's edges must rise from >= 0 to nbin %d in steps of 1 .. %d"
                         % (what, nbin, MAX_BLOCK))
    return e


class WhitenStage(PlaneStage):
    @staticmethod
    def whiten_plan(nbin, kstart=1, w0=6, wmax=128):
        """The blocks over which a spectrum of ``nbin`` bins is whitened (host
        arithmetic, integers only): the first starts at ``kstart``; the block
        at bin e is ``w = min(wmax, max(w0, e >> 3))`` bins wide -- the width
        grows in proportion to the frequency and is constant from 8 ``wmax``
        on -- and when fewer than 2 w bins are left it runs to ``nbin`` and
        ends the plan, so that the longest block stays below 2 ``wmax`` <=
        256.  ``1 <= w0 <= wmax <= 128`` and ``0 <= kstart < nbin``.  Returns
        a :class:`WhitenPlan`."""
        what = "whiten_plan"
        nb, ks, a, b = _integers(what, "nbin, kstart, w0 and wmax", nbin, kstart, w0, wmax)
        if nb < 1:
            raise ValueError("%s: nbin %d < 1" % (what, nb))
        if not (1 <= a <= b <= 128):
            raise ValueError("%s: w0 %d and wmax %d must satisfy 1 <= w0 <= wmax <= 128" % (what, a, b))
        if not (0 <= ks < nb):
            raise ValueError("%s: kstart %d outside [0, %d)" % (what, ks, nb))
        edges = [ks]
        e = ks
        while e < nb:
            w = min(b, max(a, e >> 3))
            e = nb if nb - e < 2 * w else e + w
            edges.append(e)
        return WhitenPlan(np.array(edges, dtype=np.int64), nb, ks, a, b)

    @staticmethod
    def zap_mask(nfft, samprate, ranges):
        """The interference mask of :meth:`whiten_spectrum` for a transform of
        ``nfft`` samples at ``samprate`` [MHz] (host only): uint8 [nfft // 2],
        1 at every bin whose centre k df, df = samprate / nfft, lies in one of
        the closed ``ranges`` (pairs (f_lo, f_hi) in Hz, or quantities).  A
        range outside the band sets nothing.  The mask crosses to the device
        in the call that uses it."""
        what = "zap_mask"
        (nf,) = _integers(what, "nfft", nfft)
        if nf < 2 or nf % 2:
            raise ValueError("%s: nfft %d is not an even length >= 2" % (what, nf))
        try:
            fs = float(to_value(samprate, 'MHz')) * 1e6
        except (TypeError, ValueError):
            fs = np.nan
        if not np.isfinite(fs) or fs <= 0:
            raise ValueError("%s: the sample rate %r is not finite and positive" % (what, samprate))
        centre = np.arange(nf // 2, dtype=np.int64) * (fs / nf)
        mask = np.zeros(nf // 2, dtype=np.uint8)
        try:
            pairs = [tuple(r) for r in ranges]
        except TypeError:
            pairs = [()]
        for r in pairs:
            try:
                lo, hi = (float(to_value(v, 'Hz')) for v in r)
            except (TypeError, ValueError):
                lo = hi = np.nan
            if not (np.isfinite(lo) and np.isfinite(hi) and lo <= hi):
                raise ValueError("%s: a range must be a pair (f_lo, f_hi) of finite frequencies, f_lo <= f_hi, not %r"
                                 % (what, r))
            mask[(centre >= lo) & (centre <= hi)] = 1
        return mask

    @staticmethod
    def _whiten_args(what, whiten, zap, nbin):
        """The ``whiten=`` / ``zap=`` keywords on the host: (the
        :class:`WhitenPlan` with its table checked, or None for off; the mask
        as uint8 [nbin] on the host or as a device tensor, or None)."""
        if whiten is None or whiten is False:
            if zap is not None:
                raise ValueError("%s: zap needs whiten (a neutral value of power 1 has no meaning under another "
                                 "scale)" % what)
            return None, None
        if whiten is True:
            plan = WhitenStage.whiten_plan(nbin)
        elif isinstance(whiten, dict):
            if not set(whiten) <= {"kstart", "w0", "wmax"}:
                raise ValueError("%s: whiten holds %s; whiten_plan takes kstart, w0 and wmax"
                                 % (what, ", ".join(sorted(str(k) for k in set(whiten) - {"kstart", "w0", "wmax"}))))
            plan = WhitenStage.whiten_plan(nbin, **whiten)
        elif isinstance(whiten, WhitenPlan):
            plan = whiten
        else:
            raise ValueError("%s: whiten must be None, a bool, a WhitenPlan or a dict of whiten_plan's keywords, not %s"
                             % (what, type(whiten).__name__))
        edges = _check_edges(what, plan.edges, nbin)
        if plan.edges is not edges:
            plan = WhitenPlan(edges, nbin, plan.kstart, plan.w0, plan.wmax)
        if zap is not None:
            if isinstance(zap, torch.Tensor):
                if tuple(zap.shape) != (nbin,):
                    raise ValueError("%s: zap has the shape %s for %d bins" % (what, tuple(zap.shape), nbin))
            else:
                z = np.asarray(zap)
                if z.shape != (nbin,) or z.dtype.kind not in "biu":
                    raise ValueError("%s: zap must be an integer or bool mask of %d bins" % (what, nbin))
                zap = (z != 0).astype(np.uint8)
        return plan, zap

    @staticmethod
    def _whiten_tables(plan, zap, device):
        """(edges, zap or None) on the device: uploaded, not yet fenced (the next library call fences)."""
        edges_d = _engine.to_dev(plan.edges)
        if zap is None:
            return edges_d, None
        if isinstance(zap, torch.Tensor):
            return edges_d, (zap != 0).to(device=device, dtype=torch.uint8).contiguous()
        return edges_d, _engine.to_dev(zap)

    @staticmethod
    def _whiten_rows(L, spec, nbin, plan, edges_d, zap_d, med, out=None):
        """Whiten the rows of ``spec`` (complex64, contiguous rows of at least ``nbin`` bins) into ``out``
        (default: in place) through ``med`` (float32 [>= rows][nblk]); returns ``out``."""
        n, ld = int(spec.shape[0]), int(spec.stride(0))
        out = spec if out is None else out
        rc = L.pss_spectrum_medians(_engine.ptr(spec), n, nbin, ld, _engine.ptr(edges_d), plan.nblk, _engine.ptr(med),
                                    int(med.stride(0)), _engine.stream_ptr())
        _lib.check(rc, "spectrum_medians")
        rc = L.pss_spectrum_whiten(_engine.ptr(spec), n, nbin, ld, _engine.ptr(edges_d), plan.nblk, _engine.ptr(med),
                                   int(med.stride(0)), _engine.ptr(zap_d), _engine.ptr(out), int(out.stride(0)),
                                   _engine.stream_ptr())
        _lib.check(rc, "spectrum_whiten")
        return out

    @staticmethod
    def _whiten_spectrum_args(what, spectrum, plan, zap):
        """(spectrum as contiguous complex64 on its device, the plan, the mask) of the two calls that take a spectrum."""
        if not isinstance(spectrum, torch.Tensor) or spectrum.dim() != 2 or int(spectrum.shape[0]) < 1 \
                or int(spectrum.shape[1]) < 2:
            raise ValueError("%s takes a spectrum [nDM, nfft // 2 + 1] on the device" % what)
        nbin = int(spectrum.shape[1]) - 1
        plan, zap = WhitenStage._whiten_args(what, True if plan is None else plan, zap, nbin)
        return nbin, plan, zap

    def spectrum_medians(self, spectrum, plan=None):
        """The noise spectrum of every trial on the device (extension: the
        reference has no counterpart): the lower median of the power |X|^2
        over every block of ``plan`` (a :class:`WhitenPlan`; default
        :meth:`whiten_plan` (nbin), nbin = spectrum.shape[1] - 1, the
        convention of :meth:`dm_spectrum`), float32 [nDM, nblk]
        (``pss_spectrum_medians``, include/pss_hip.h: a selection, exact).  The
        median of the power of white noise is its mean times ln 2.  No host
        synchronisation."""
        nbin, plan, _ = self._whiten_spectrum_args("spectrum_medians", spectrum, plan, None)
        spec = spectrum
        if spec.dtype != torch.complex64 or not spec.is_contiguous():
            spec = spec.to(torch.complex64).contiguous()
        edges_d, _ = self._whiten_tables(plan, None, spec.device)
        med = torch.empty((int(spec.shape[0]), plan.nblk), dtype=torch.float32, device=spec.device)
        rc = _lib.lib().pss_spectrum_medians(_engine.ptr(spec), int(spec.shape[0]), nbin, int(spec.stride(0)),
                                             _engine.ptr(edges_d), plan.nblk, _engine.ptr(med), plan.nblk,
                                             _engine.stream_ptr())
        _lib.check(rc, "spectrum_medians")
        return med

    def whiten_spectrum(self, spectrum, plan=None, zap=None, inplace=False):
        """Whiten the spectrum of every trial on the device (extension: the
        reference has no counterpart; what PRESTO's ``rednoise`` and
        ``zapbirds`` do between the transform and the search).  Every bin is
        multiplied by ``sqrt(ln 2 / norm)``, norm the block medians of
        :meth:`spectrum_medians` interpolated linearly between the block
        centres (``pss_spectrum_whiten``, include/pss_hip.h), so that the power
        of noise has unit mean whatever its colour and ``pss_harmonic_search``
        takes the result with a scale of 1.  The bins below the plan's
        ``kstart`` are zeroed; a bin set in ``zap`` (uint8 [nbin] from
        :meth:`zap_mask`, any array or a device tensor) becomes (1, 0), the
        mean power exactly.  The Nyquist bin is left as it is.  Returns
        complex64 [nDM, nfft // 2 + 1]: a new tensor, or with ``inplace`` the
        spectrum itself (it must then be contiguous complex64).  The same bits
        either way.  No host synchronisation."""
        what = "whiten_spectrum"
        nbin, plan, zap = self._whiten_spectrum_args(what, spectrum, plan, zap)
        spec = spectrum
        if inplace:
            if spec.dtype != torch.complex64 or not spec.is_contiguous():
                raise ValueError("%s: in place takes a contiguous complex64 spectrum" % what)
            out = spec
        else:
            if spec.dtype != torch.complex64 or not spec.is_contiguous():
                spec = spec.to(torch.complex64).contiguous()
            out = torch.empty_like(spec)
            out[:, nbin:] = spec[:, nbin:]
        edges_d, zap_d = self._whiten_tables(plan, zap, spec.device)
        med = torch.empty((int(spec.shape[0]), plan.nblk), dtype=torch.float32, device=spec.device)
        self._whiten_rows(_lib.lib(), spec, nbin, plan, edges_d, zap_d, med, out)
        return out
