"""Acceleration search: the periodicity search over trial accelerations (time-domain resampling)."""
from fractions import Fraction

import numpy as np
import torch

from .._units import to_value
from .. import _engine, _lib
from .plane import PlaneStage, Candidates, _check_plane
from .periodicity import HarmonicPlane, PERIOD_DTYPE

C_M_S = 299792458.0                      # speed of light, m/s (exact)


class AccelPlane(HarmonicPlane):
    """Result of :meth:`Backend.accel_snr`: per cell of every trial the best
    harmonic sum over the trial accelerations, on the device.  The fields of
    :class:`HarmonicPlane` (``snr``, ``bin``, ``nharm_log2``, ``code``,
    ``freq`` ... of the winning acceleration), and

    ``acc_index``  torch int32 [nDM, nq], the index into ``accels`` of the
                   acceleration that won the cell (the one given first on a
                   tie; 0 where ``snr`` is -inf)
    ``accels``     the trial accelerations, float64 [nacc] (m/s^2)"""
    whiten = None

    def __init__(self, snr, bin, nharm_log2, code, freq, df, nfft, nbin, kmin, cell, mean, std, plane, acc_index,
                 accels):
        HarmonicPlane.__init__(self, snr, bin, nharm_log2, code, freq, df, nfft, nbin, kmin, cell, mean, std, plane)
        self.acc_index = acc_index
        self.accels = accels

    def __repr__(self):
        return "AccelPlane(%d trials x %d cells of %d bins, %d accelerations, df %.6g Hz)" % (
            self.snr.shape[0], self.snr.shape[1], self.cell, len(self.accels), self.df)


ACCEL_DTYPE = np.dtype(PERIOD_DTYPE.descr + [("accel", np.float64), ("acc_index", np.int32)])


class AccelCandidates(Candidates):
    """Result of :meth:`Backend.accel_search`: the fields of
    :class:`PeriodCandidates` (same order, same meaning) plus ``accel`` (m/s^2)
    and ``acc_index``, the trial acceleration of the candidate's winning cell.
    ``array`` is the NumPy structured array (``ACCEL_DTYPE``), ``cells`` the
    :class:`AccelPlane` and ``threshold`` the cut."""
    _dtype = ACCEL_DTYPE


class AccelStage(PlaneStage):
    @staticmethod
    def _accel_alpha(accel, samprate):
        """alpha = -a / (2 c fs) per sample as an exact Fraction of the float64
        inputs (fs = samprate [MHz] * 1e6, the float64 product)."""
        a = float(accel)
        fs = float(to_value(samprate, 'MHz')) * 1e6
        if not np.isfinite(a):
            raise ValueError("acceleration search: the acceleration %r is not finite" % (accel,))
        if not np.isfinite(fs) or fs <= 0:
            raise ValueError("acceleration search: the sample rate %r is not finite and positive" % (samprate,))
        return -Fraction(a) / (2 * Fraction(C_M_S) * Fraction(fs))

    @staticmethod
    def accel_shift_step(accel, samprate, T):
        """The table entry ``kappa`` of :meth:`accel_resample` and
        ``pss_accel_resample`` for a line-of-sight acceleration ``accel``
        [m/s^2] (host only).  Positive is acceleration away from the observer:
        the observed spin frequency falls as f0 (1 - a t / c).  A series of
        ``T`` samples at ``samprate`` [MHz] is then read at t + alpha t (T - t),

            alpha = -a / (2 c fs)  per sample,   fs = samprate 1e6 Hz,
            kappa = sign(alpha) floor(|alpha| 2^64 + 1/2),

        the mid-observation shift being alpha T^2 / 4 samples.  Computed with
        ``fractions.Fraction`` on the float64 inputs: no float rounding enters
        an index.  ValueError when |alpha| T > 1/2 (the kernel's bound: beyond
        it the map would no longer be monotone).  Returns a signed Python
        int."""
        T = int(T)
        if T < 1:
            raise ValueError("acceleration search: T %d < 1" % T)
        al = AccelStage._accel_alpha(accel, samprate)
        if abs(al) * T > Fraction(1, 2):
            raise ValueError("acceleration search: |a| = %g m/s^2 shifts by more than T / 8 samples (|alpha| T = %g "
                             "> 1/2)" % (abs(float(accel)), float(abs(al) * T)))
        q = abs(al) * (1 << 64) + Fraction(1, 2)
        k = q.numerator // q.denominator
        return k if al >= 0 else -k

    @staticmethod
    def accel_trials(T, samprate, amax, tol=1.0):
        """The trial accelerations [m/s^2] for a series of ``T`` samples at
        ``samprate`` [MHz]: the ascending float64 grid i da, |i| <= ceil(amax /
        da), da = 8 c fs tol / T^2 -- neighbouring trials differ by ``tol``
        samples at mid-observation.  Always contains 0 (host only)."""
        T = int(T)
        fs = float(to_value(samprate, 'MHz')) * 1e6
        am, tl = float(amax), float(tol)
        if T < 1 or not np.isfinite(fs) or fs <= 0:
            raise ValueError("accel_trials: T %d and the sample rate %r must be positive" % (T, samprate))
        if not np.isfinite(am) or am < 0 or not np.isfinite(tl) or tl <= 0:
            raise ValueError("accel_trials: amax %r must be finite and >= 0, tol %r finite and > 0" % (amax, tol))
        da = 8.0 * C_M_S * fs * tl / (float(T) * float(T))
        n = int(np.ceil(am / da))
        return np.arange(-n, n + 1, dtype=np.float64) * da

    @staticmethod
    def _accel_kappas(accels, samprate, T, what):
        """(accels float64 [nacc], kappa int64 [nacc]) after validation."""
        acc = np.atleast_1d(np.asarray(accels, dtype=np.float64))
        if acc.ndim != 1 or acc.size < 1 or not np.all(np.isfinite(acc)):
            raise ValueError("%s: accels must hold at least one finite acceleration" % what)
        kap = [AccelStage.accel_shift_step(a, samprate, T) for a in acc]
        # (T = 1 alone reaches 2^63; u(t) = 0 there)
        return acc, np.array([min(k, (1 << 63) - 1) for k in kap], dtype=np.int64)

    @staticmethod
    def _accel_launch(L, data, ndm, T, ld, src_d, kap_d, sub_d, nrows, n_out, out, out_ld):
        rc = L.pss_accel_resample(_engine.ptr(data), ndm, T, ld, _engine.ptr(src_d), _engine.ptr(kap_d),
                                  _engine.ptr(sub_d), nrows, n_out, _engine.ptr(out), out_ld, _engine.stream_ptr())
        _lib.check(rc, "accel_resample")

    def accel_resample(self, plane, accels, trials=None, mean=None, n_out=None):
        """Resample every trial of a DM-time plane for every trial
        acceleration on the device (extension: the reference has no
        counterpart): row (j, a) is trial j read at the stretched times
        t + alpha_a t (T - t) of :meth:`accel_shift_step` (accels[a],
        plane.samprate, T), rounded to whole samples with integers
        (``pss_accel_resample``, include/pss_hip.h), minus float32(mean[j]) --
        which straightens a pulse train of that acceleration.  Returns the
        device tensor float32 [nDM', nacc, ``n_out``] (default T; the map does
        not depend on it), rows on the 16-B grid.  ``mean`` is as in
        :meth:`dm_spectrum` (default: the block-median mean), ``trials`` = (lo,
        hi) restricts the rows to trials lo .. hi - 1.  One src / kappa table
        crosses to the device per call; no host synchronisation."""
        what = "accel_resample"
        ndm, T = _check_plane(what, plane)
        data, ld = self._plane_rows(plane.data)
        if ndm < 1 or T < 1:
            raise ValueError("%s: the plane is empty" % what)
        acc, kap = self._accel_kappas(accels, plane.samprate, T, what)
        n = T if n_out is None else int(n_out)
        if not (1 <= n <= T):
            raise ValueError("%s: n_out %d outside [1, %d]" % (what, n, T))
        lo, hi = (0, ndm) if trials is None else (int(trials[0]), int(trials[1]))
        if not (0 <= lo < hi <= ndm):
            raise ValueError("%s: trials (%d, %d) outside [0, %d]" % (what, lo, hi, ndm))
        mean_d = self._trial_mean(data, ld, ndm, mean, 1024, what)
        na, nt = acc.size, hi - lo
        src_d = _engine.to_dev(np.repeat(np.arange(lo, hi, dtype=np.int32), na))
        kap_d = _engine.to_dev(np.tile(kap, nt))
        _engine.wait_uploads()
        sub_d = mean_d.to(torch.float32)[lo:hi].repeat_interleave(na)
        out_ld = (n + 3) // 4 * 4
        out = torch.empty((nt, na, out_ld), dtype=torch.float32, device=data.device)
        self._accel_launch(_lib.lib(), data, ndm, T, ld, src_d, kap_d, sub_d, nt * na, n, out, out_ld)
        return out[:, :, :n]

    def accel_snr(self, plane, accels, nharm=16, cell=32, nfft=None, fmin=None, mean=None, std=None,
                  stat_block=1024, max_bytes=1 << 30, whiten=None, zap=None):
        """:meth:`harmonic_snr` maximised over trial accelerations, on the
        device (extension: the reference has no counterpart).  Every trial is
        resampled in the time domain for every entry of ``accels`` [m/s^2]
        (:meth:`accel_resample`: ``pss_accel_resample`` writes straight into
        the min(T, nfft) samples the transform takes, the float32 mean
        subtracted in the kernel), transformed (``torch.fft.rfft(n=nfft)``) and
        searched (``pss_harmonic_search``, the trial's scale repeated for its
        accelerations), in chunks of rows whose resampled series, spectrum and
        power workspace stay within ``max_bytes``.  Per (trial, cell) the
        running maximum over the accelerations is kept on the device -- a tie
        goes to the acceleration given first -- and the full [nDM, nacc, nq]
        map never exists; the maps do not depend on the chunking.  The other
        arguments are those of :meth:`harmonic_snr`.

        ``mean`` / ``std`` are given, or the block medians of the *original*
        trial, measured once: a resampled series repeats or drops at most
        2 s_max of the trial's T samples (s_max the mid-observation shift), so
        its statistics are the trial's to that fraction.  ``accels`` must be
        finite, at least one, and within the limit of
        :meth:`accel_shift_step`.  ``accels = [0.0]`` gives the maps of
        :meth:`harmonic_snr`.  ``whiten`` / ``zap`` are those of
        :meth:`harmonic_snr`: every chunk of spectra is whitened in place
        straight after the transform and searched with a scale of ones
        (``std`` is still reported but does not enter the normalisation).  No
        host synchronisation.  Returns an :class:`AccelPlane`."""
        p = self._harmonic_plan(plane, nharm=nharm, cell=cell, nfft=nfft, fmin=fmin, mean=mean, std=std,
                                stat_block=stat_block, max_bytes=max_bytes, whiten=whiten, zap=zap)
        ndm, T, ce, nbin, nu = p["ndm"], p["T"], p["cell"], p["nbin"], p["n_used"]
        acc, kap = self._accel_kappas(accels, plane.samprate, T, "accel_snr")
        na = acc.size
        # a row's resampled series, its spectrum, and its powers with 8 or 16 harmonics
        # (rows on the 16-B grid: the kernel's 16-B stores at every transform length)
        y_ld = (nu + 3) // 4 * 4
        per_row = y_ld * 4 + (nbin + 1) * 8 + (nbin * 4 if p["nl"] > 3 else 0)
        rows = int(max_bytes) // per_row
        if rows < 1:
            raise ValueError("accel_snr: max_bytes %d is below one resampled row with its spectrum (%d bytes)"
                             % (int(max_bytes), per_row))
        data, ld = self._plane_rows(plane.data)
        dev = data.device
        mean_d, std_d, scale32 = self._harmonic_stats(data, ld, p)
        wplan = p["whiten"]
        if wplan is not None:
            edges_d, zap_d = self._whiten_tables(wplan, p["zap"], dev)
            scale32 = torch.ones(ndm, dtype=torch.float32, device=dev)
        # chunks: whole trials with all their accelerations, or one trial and a block of accelerations
        nt_c, na_c = (min(ndm, rows // na), na) if rows >= na else (1, rows)
        chunks = [(lo, min(ndm, lo + nt_c), a0, min(na, a0 + na_c))
                  for lo in range(0, ndm, nt_c) for a0 in range(0, na, na_c)]
        # one table for the call, the chunks' rows one after the other (trial-major, acceleration fastest)
        src_d = _engine.to_dev(np.concatenate([np.repeat(np.arange(lo, hi, dtype=np.int32), a1 - a0)
                                               for lo, hi, a0, a1 in chunks]))
        kap_d = _engine.to_dev(np.concatenate([np.tile(kap[a0:a1], hi - lo) for lo, hi, a0, a1 in chunks]))
        _engine.wait_uploads()
        mean32 = mean_d.to(torch.float32)
        nq = (nbin + ce - 1) // ce
        out_ld = (nq + 15) // 16 * 16                          # rows of whole 64-B segments
        best = torch.full((ndm, out_ld), -np.inf, dtype=torch.float32, device=dev)
        bcode = torch.zeros((ndm, out_ld), dtype=torch.int32, device=dev)
        bacc = torch.zeros((ndm, out_ld), dtype=torch.int32, device=dev)
        mrows = nt_c * na_c
        y = torch.empty((mrows, y_ld), dtype=torch.float32, device=dev)
        snr_c = torch.empty((mrows, out_ld), dtype=torch.float32, device=dev)
        code_c = torch.empty((mrows, out_ld), dtype=torch.int32, device=dev)
        work = torch.empty(mrows * nbin, dtype=torch.float32, device=dev) if p["nl"] > 3 else None
        med = torch.empty((mrows, wplan.nblk), dtype=torch.float32, device=dev) if wplan is not None else None
        L = _lib.lib()
        r0 = 0
        for lo, hi, a0, a1 in chunks:
            nt, nb = hi - lo, a1 - a0
            n = nt * nb
            self._accel_launch(L, data, ndm, T, ld, src_d[r0:r0 + n], kap_d[r0:r0 + n],
                               mean32[lo:hi].repeat_interleave(nb), n, nu, y, y_ld)
            spec = torch.fft.rfft(y[:n, :nu], n=p["nfft"])
            if wplan is not None:
                self._whiten_rows(L, spec, nbin, wplan, edges_d, zap_d, med)
            rc = L.pss_harmonic_search(_engine.ptr(spec), n, nbin, int(spec.shape[1]),
                                       _engine.ptr(scale32[lo:hi].repeat_interleave(nb)), p["nl"], p["kmin"], ce,
                                       _engine.ptr(snr_c), _engine.ptr(code_c), out_ld, _engine.ptr(work),
                                       _engine.stream_ptr())
            _lib.check(rc, "harmonic_search")
            del spec
            # the chunk's own maximum over its accelerations, the first on a tie ...
            s3, c3 = snr_c[:n].view(nt, nb, out_ld), code_c[:n].view(nt, nb, out_ld)
            top = s3.amax(dim=1)
            ai = torch.arange(nb, dtype=torch.int64, device=dev)[None, :, None]
            first = torch.where(s3 == top[:, None, :], ai, nb).amin(dim=1)
            first = torch.clamp(first, max=nb - 1)               # (a NaN never is stored; -inf equals -inf)
            ctop = torch.gather(c3, 1, first[:, None, :])[:, 0]
            # ... joins the running maximum: an earlier block keeps a tie
            better = top > best[lo:hi]
            best[lo:hi] = torch.where(better, top, best[lo:hi])
            bcode[lo:hi] = torch.where(better, ctop, bcode[lo:hi])
            bacc[lo:hi] = torch.where(better, (first + a0).to(torch.int32), bacc[lo:hi])
            r0 += n
        snr, code, bacc = best[:, :nq], bcode[:, :nq], bacc[:, :nq]
        k, lev, freq = self._decode_cells(code, ce, p["df"])
        cells = AccelPlane(snr, k, lev, code, freq, p["df"], p["nfft"], nbin, p["kmin"], ce, mean_d, std_d, plane,
                           bacc, acc)
        if wplan is not None:
            cells.whiten = wplan
        return cells

    def accel_search(self, plane, accels=None, amax=None, threshold=10.0, nharm=16, cell=32, dm_tol=1,
                     freq_tol=1.0, max_cells=1 << 20, nfft=None, fmin=None, mean=None, std=None, stat_block=1024,
                     max_bytes=1 << 30, tol=1.0, whiten=None, zap=None):
        """Acceleration search of a DM-time plane (extension: the reference has
        no counterpart): :meth:`accel_snr` over the trial accelerations, then
        the cells with ``snr >= threshold`` -- found on the device, only they
        cross to the host -- clustered on (trial, fundamental) exactly as
        :meth:`periodicity_search` does; each candidate takes the acceleration
        of its winning cell.  Give either ``accels`` [m/s^2] or ``amax``, which
        goes through :meth:`accel_trials` (T, plane.samprate, amax, ``tol``).

        ``log_fap`` is still the single-trial false-alarm probability of
        :meth:`periodicity_search`: multiply the probability by the number of
        (trial, bin, level) searched and by the number of accelerations as
        well.  ``whiten`` / ``zap`` are those of :meth:`harmonic_snr`.
        Returns :class:`AccelCandidates`."""
        if (accels is None) == (amax is None):
            raise ValueError("accel_search: give either accels or amax")
        p = self._harmonic_plan(plane, nharm, cell, nfft, fmin, threshold, dm_tol, freq_tol, max_cells, mean, std,
                                stat_block, max_bytes, None, whiten, zap)
        if accels is None:
            accels = self.accel_trials(p["T"], plane.samprate, amax, tol)
        cells = self.accel_snr(plane, accels, nharm=nharm, cell=cell, nfft=nfft, fmin=fmin, mean=mean, std=std,
                               stat_block=stat_block, max_bytes=max_bytes, whiten=whiten, zap=zap)
        base, packed = self._period_cells("accel_search", plane, cells, p, cells.acc_index)
        arr = np.empty(base.size, dtype=ACCEL_DTYPE)
        for name in PERIOD_DTYPE.names:
            arr[name] = base[name]
        # a candidate is one of the cells: (trial, cell) finds it again
        nq = int(cells.snr.shape[1])
        key = packed[0] * nq + packed[1] // p["cell"]
        order = np.argsort(key, kind="stable")
        pos = order[np.searchsorted(key[order], base["dm_index"].astype(np.int64) * nq + base["bin"] // p["cell"])] \
            if base.size else np.zeros(0, dtype=np.int64)
        arr["acc_index"] = packed[3][pos]
        arr["accel"] = cells.accels[packed[3][pos]]
        return AccelCandidates(arr, cells, p["threshold"])
