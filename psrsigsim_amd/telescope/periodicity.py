"""Periodicity search: harmonic sums of the plane's power spectrum, thresholded and clustered."""
import numpy as np
import torch

from .._units import to_value
from .. import _engine, _lib
from .plane import (PlaneStage, Candidates, cluster_cells, _cluster_candidates, _check_plane, _integers, _check_cells,
                    _threshold, _given_stats)
from .whiten import WhitenStage


class HarmonicPlane(object):
    """Result of :meth:`Backend.harmonic_snr`: the best harmonic sum of every
    cell of ``cell`` spectral bins of every trial, on the device
    (nq = ceil(nbin / cell)).

    ``snr``        torch float32 [nDM, nq], -inf where a cell holds no candidate
    ``bin``        torch int64 [nDM, nq], the bin k of the highest harmonic of
                   the winning sum
    ``nharm_log2`` torch int32 [nDM, nq], it sums 2**nharm_log2 harmonics
    ``code``       torch int32 [nDM, nq], the kernel's (l << 16) | (k - q * cell)
    ``freq``       torch float64 [nDM, nq], the fundamental in Hz, bin / 2^l * df
    ``df``         width of a bin in Hz, samprate / nfft
    ``nfft``       length of the transform (the series is cut or zero-padded to it)
    ``nbin``       bins searched, nfft // 2 (the Nyquist bin is left out)
    ``kmin``       lowest bin a fundamental may have
    ``cell``       bins per cell
    ``mean``       torch float64 [nDM], the baseline subtracted from each trial
    ``std``        torch float64 [nDM], the noise of one sample of each trial
                   (0: a trial without a usable variance, its power is 0)
    ``plane``      the :class:`DedispersedPlane` that was searched
    ``whiten``     None, or the :class:`WhitenPlan` the spectrum was whitened
                   with (``std`` then did not enter the normalisation)"""
    whiten = None

    def __init__(self, snr, bin, nharm_log2, code, freq, df, nfft, nbin, kmin, cell, mean, std, plane):
        self.snr = snr
        self.bin = bin
        self.nharm_log2 = nharm_log2
        self.code = code
        self.freq = freq
        self.df = df
        self.nfft = nfft
        self.nbin = nbin
        self.kmin = kmin
        self.cell = cell
        self.mean = mean
        self.std = std
        self.plane = plane

    def __repr__(self):
        return "HarmonicPlane(%d trials x %d cells of %d bins, df %.6g Hz)" % (
            self.snr.shape[0], self.snr.shape[1], self.cell, self.df)


PERIOD_DTYPE = np.dtype([("snr", np.float32), ("dm_index", np.int32), ("dm", np.float64), ("bin", np.int64),
                         ("nharm", np.int32), ("freq", np.float64), ("period", np.float64),
                         ("log_fap", np.float64), ("ncells", np.int64)])


class PeriodCandidates(Candidates):
    """Result of :meth:`Backend.periodicity_search`: one candidate per cluster
    of cells above the threshold, on the host, ordered by ``snr`` descending,
    then (``dm_index``, ``bin``, ``nharm``) ascending.

    ``array`` is the NumPy structured array (``PERIOD_DTYPE``); every field is
    also an attribute: ``snr`` (the harmonic sum in units of its own standard
    deviation), ``dm_index``, ``dm`` (pc/cm^3), ``bin`` (of the highest
    harmonic), ``nharm`` (harmonics summed), ``freq`` (the fundamental, Hz),
    ``period`` (s), ``log_fap`` (natural logarithm of the single-trial
    false-alarm probability of ``snr`` in white noise) and ``ncells`` (cells of
    the cluster).  ``cells`` is the :class:`HarmonicPlane` and ``threshold``
    the cut."""
    _dtype = PERIOD_DTYPE


def harmonic_log_fap(snr, nharm):
    """ln of the probability that the sum of ``nharm`` exp(1) powers, in units
    of its own standard deviation, reaches ``snr`` in one trial: twice the sum
    H = snr sqrt(h) + h is chi-square with 2h degrees of freedom.  At h = 1
    this is -(snr + 1): the sum of a few exponentials is far from Gaussian."""
    from scipy.stats import chi2
    h = np.asarray(nharm, dtype=np.float64)
    return chi2.logsf(2.0 * (np.asarray(snr, dtype=np.float64) * np.sqrt(h) + h), 2.0 * h)


def period_candidates_from_cells(snr, dm_index, bin, level, dms, df, dm_tol=1, freq_tol=1.0):
    """Cluster the cells (``dm_index``, fundamental ``bin / 2^level`` bins)
    with :func:`cluster_cells` -- on F = bin 2^(4 - level), the fundamental in
    sixteenths of a bin (an exact integer), width 0 and a tolerance of
    round(16 freq_tol) -- and return the structured array of one candidate per
    cluster, its lexicographic maximum of (snr, -dm_index, -bin), in the order
    of :class:`PeriodCandidates`."""
    snr = np.asarray(snr, dtype=np.float32)
    j = np.asarray(dm_index, dtype=np.int64)
    k = np.asarray(bin, dtype=np.int64)
    lev = np.asarray(level, dtype=np.int64)
    F = np.left_shift(k, 4 - lev)
    labels = cluster_cells(j, F, np.zeros_like(F), dm_tol, int(round(16 * float(freq_tol))))
    out, best = _cluster_candidates(PERIOD_DTYPE, labels, snr, j, k, dms)
    out["bin"] = k[best]
    out["nharm"] = np.left_shift(1, lev[best])
    out["freq"] = k[best] / np.left_shift(1, lev[best]).astype(np.float64) * float(df)
    with np.errstate(divide="ignore"):
        out["period"] = 1.0 / out["freq"]
    out["log_fap"] = harmonic_log_fap(out["snr"], out["nharm"]) if best.size else 0.0
    final = np.lexsort((out["nharm"], out["bin"], out["dm_index"], -out["snr"].astype(np.float64)))
    return out[final]


class PeriodicityStage(PlaneStage):
    @staticmethod
    def fft_length(T):
        """The largest even n <= T of the form 2^a 3^b 5^c: a transform length
        the FFT library handles with its fast radices (host arithmetic)."""
        T = int(T)
        if T < 2:
            raise ValueError("fft_length: no even length fits %d samples" % T)
        best = 2
        p5 = 1
        while 2 * p5 <= T:
            p3 = p5
            while 2 * p3 <= T:
                n = 2 * p3
                while 2 * n <= T:
                    n *= 2
                best = max(best, n)
                p3 *= 3
            p5 *= 5
        return best

    @staticmethod
    def _harmonic_plan(plane, nharm=16, cell=32, nfft=None, fmin=None, threshold=10.0, dm_tol=1, freq_tol=1.0,
                       max_cells=1 << 20, mean=None, std=None, stat_block=1024, max_bytes=1 << 30, spectrum=None,
                       whiten=None, zap=None):
        """Validate the arguments of :meth:`dm_spectrum`, :meth:`harmonic_snr`
        and :meth:`periodicity_search` on the host (nothing touches the
        device): returns a dict with ndm, T, nl (levels, log2(nharm) + 1), cell,
        nfft, nbin, n_used (samples of a trial that enter the transform), df
        (Hz), kmin, threshold, dm_tol, freq_tol, max_cells, mean, std (float64
        [nDM] or None), stat_block, chunk (trials per spectrum chunk), whiten
        (the :class:`WhitenPlan`, or None for off) and zap (the mask, or
        None)."""
        what = "periodicity search"
        ndm, T = _check_plane(what, plane, 2, "too small")
        nh, ce, sb, mc, mb, nf = _integers(what, "nharm, cell, nfft, stat_block, max_cells and max_bytes", nharm, cell,
                                           stat_block, max_cells, max_bytes, 0 if nfft is None else nfft)
        nf = None if nfft is None else nf
        if nh not in (1, 2, 4, 8, 16):
            raise ValueError("%s: nharm %d is not one of 1, 2, 4, 8, 16" % (what, nh))
        _check_cells(what, ce, sb, mc)
        if spectrum is not None:
            shp = tuple(int(s) for s in spectrum.shape)
            if len(shp) != 2 or shp[0] != ndm or shp[1] < 2:
                raise ValueError("%s: spectrum has the shape %s for %d trials" % (what, "x".join(map(str, shp)), ndm))
            if nf is None:
                nf = 2 * (shp[1] - 1)
            elif shp[1] != nf // 2 + 1:
                raise ValueError("%s: spectrum has %d bins, nfft %d gives %d" % (what, shp[1], nf, nf // 2 + 1))
        if nf is None:
            nf = PeriodicityStage.fft_length(T)
        if nf < 2 or nf % 2:
            raise ValueError("%s: nfft %d is not an even length >= 2" % (what, nf))
        nbin = nf // 2
        if nbin > 1 << 27:
            raise ValueError("%s: nfft %d gives more than 2^27 bins" % (what, nf))
        per_trial = (nbin + 1) * 8
        if mb < per_trial:
            raise ValueError("%s: max_bytes %d is below one trial's spectrum (%d bytes)" % (what, mb, per_trial))
        df = float(plane.samprate) * 1e6 / nf
        if fmin is None:
            kmin = 1
        else:
            try:
                fm = float(to_value(fmin, 'Hz'))
            except (TypeError, ValueError):
                fm = np.nan
            if not np.isfinite(fm) or fm < 0:
                raise ValueError("%s: fmin %r is not a finite frequency >= 0" % (what, fmin))
            kmin = max(1, int(np.ceil(fm / df)))
        th = _threshold(what, threshold, dm_tol, "freq_tol", freq_tol)
        mean, std = _given_stats(what, mean, std, ndm)
        wplan, zap = WhitenStage._whiten_args(what, whiten, zap, nbin)
        return dict(ndm=ndm, T=T, nl=nh.bit_length(), cell=ce, nfft=nf, nbin=nbin, n_used=min(T, nf), df=df,
                    kmin=kmin, threshold=th, dm_tol=dm_tol, freq_tol=freq_tol, max_cells=mc, mean=mean, std=std,
                    stat_block=sb, chunk=max(1, min(ndm, mb // per_trial)), whiten=wplan, zap=zap)

    def dm_spectrum(self, plane, nfft=None, mean=None, trials=None):
        """The complex spectrum of every trial of a DM-time plane on the
        device: ``torch.fft.rfft(data[:, :min(T, nfft)] - mean32[:, None],
        n=nfft)``, complex64 [nDM', nfft // 2 + 1].  ``nfft`` (even; default
        :meth:`fft_length` (T)) cuts the series or pads it with zeros;
        ``nfft = 2 T`` halves the scalloping loss between bins.  ``mean``
        (scalar, array-like of length nDM or a device tensor; default: the
        block-median mean of :meth:`boxcar_snr`) is subtracted in float32
        before the transform so that bin 0 does not leak.  ``trials`` = (lo,
        hi) restricts the rows to trials lo .. hi - 1.  The transform is the
        FFT library's, through torch."""
        p = self._harmonic_plan(plane, nfft=nfft)
        data, ld = self._plane_rows(plane.data)
        mean_d = self._trial_mean(data, ld, p["ndm"], mean, p["stat_block"], "dm_spectrum")
        lo, hi = (0, p["ndm"]) if trials is None else (int(trials[0]), int(trials[1]))
        if not (0 <= lo < hi <= p["ndm"]):
            raise ValueError("dm_spectrum: trials (%d, %d) outside [0, %d]" % (lo, hi, p["ndm"]))
        _engine.wait_uploads()                                 # (a mean from the host)
        return self._spectrum_rows(data, mean_d.to(torch.float32), lo, hi, p["n_used"], p["nfft"])

    def _harmonic_stats(self, data, ld, p):
        """(mean, std float64 [nDM], scale float32 [nDM]) on the device, uploads fenced: given (``p``) or measured."""
        if p["mean"] is not None:
            mean_d, std_d = _engine.to_dev(p["mean"]), _engine.to_dev(p["std"])
            with np.errstate(all="ignore"):
                scale32 = _engine.to_dev((1.0 / (p["std"] * p["std"] * p["n_used"])).astype(np.float32))
            _engine.wait_uploads()
        else:
            mean_d, var = self._trial_stats(data, ld, p["stat_block"])
            good = torch.isfinite(var) & (var > 0)
            std_d = torch.where(good, torch.sqrt(var), torch.zeros_like(var))
            # (from the std that is reported, as with user-given statistics)
            scale32 = torch.where(good, 1.0 / (std_d * std_d * p["n_used"]), torch.zeros_like(var)).to(torch.float32)
        return mean_d, std_d, scale32

    def _decode_cells(self, code, cell, df):
        """The kernel's ``code`` [nDM, nq] as the winning (bin int64, nharm_log2 int32, freq float64 Hz)."""
        k, lev = self._cell_entries(code, cell)
        return k, lev, k.to(torch.float64) / torch.bitwise_left_shift(torch.ones_like(k), lev.to(torch.int64)) * df

    @staticmethod
    def _spectrum_rows(data, mean32, lo, hi, n_used, nfft):
        return torch.fft.rfft(data[lo:hi, :n_used] - mean32[lo:hi, None], n=nfft)

    def harmonic_snr(self, plane, nharm=16, cell=32, nfft=None, fmin=None, mean=None, std=None, stat_block=1024,
                     max_bytes=1 << 30, spectrum=None, whiten=None, zap=None):
        """Incoherent harmonic sums of the power spectrum of a DM-time plane on
        the device (extension: the reference has no counterpart).  Every trial
        is transformed (:meth:`dm_spectrum`), its power normalised to unit mean
        in white noise -- ``P = |X|^2 scale``, ``scale = float32(1 / (std^2
        min(T, nfft)))`` -- and for every bin k < nbin = nfft // 2 and every
        level l <= log2(``nharm``) the sum over m = 1 .. h = 2^l of the power
        at the bin nearest to k m / h,

            z = (sum - h) / sqrt(h)

        in float32 in the fixed order of ``pss_harmonic_search``
        (include/pss_hip.h); k is the bin of the highest harmonic, the
        fundamental sits at k / h bins and must be at least ``kmin = max(1,
        ceil(fmin / df))``.  Per cell of ``cell`` (a power of two in [16,
        2048]) bins the largest z is kept -- ties to the fewer harmonics, then
        the lower bin.  Returns a :class:`HarmonicPlane`.

        ``mean`` / ``std`` are as in :meth:`boxcar_snr`: given, or the block
        medians measured on the device; a trial whose variance is not positive
        and finite gets scale 0.  The trials are transformed in chunks whose
        spectrum stays within ``max_bytes`` (with 8 or 16 harmonics the
        kernel's power pass takes half as much again as workspace); the maps do
        not depend on the chunking.  ``spectrum`` (from :meth:`dm_spectrum`, all trials) skips
        the transform.

        ``whiten`` (None / False: off; True: :meth:`whiten_plan` (nbin); a
        :class:`WhitenPlan`; or a dict of :meth:`whiten_plan`'s keywords)
        whitens every spectrum chunk in place straight after the transform
        (:meth:`whiten_spectrum`: block medians of the power, red noise) and
        hands the kernel a scale of ones: ``mean`` is used as before, ``std``
        is still measured or taken and reported, but does not enter the
        normalisation.  A caller's ``spectrum`` is whitened into a copy and
        left alone: that path takes one more spectrum of all trials in device
        memory, outside ``max_bytes`` (a spectrum that had to be converted to
        contiguous complex64 is a copy already and is whitened in place).
        ``zap`` (:meth:`zap_mask`, an array or a device tensor of
        nbin entries) replaces the bins it sets by the neutral value of power
        1; it needs ``whiten``.  The plan used is the result's ``whiten``.  No
        host synchronisation."""
        p = self._harmonic_plan(plane, nharm=nharm, cell=cell, nfft=nfft, fmin=fmin, mean=mean, std=std,
                                stat_block=stat_block, max_bytes=max_bytes, spectrum=spectrum, whiten=whiten, zap=zap)
        ndm, ce, nbin = p["ndm"], p["cell"], p["nbin"]
        data, ld = self._plane_rows(plane.data)
        mean_d, std_d, scale32 = self._harmonic_stats(data, ld, p)
        mean32 = mean_d.to(torch.float32)
        nq = (nbin + ce - 1) // ce
        out_ld = (nq + 15) // 16 * 16                          # rows of whole 64-B segments
        snr = torch.empty((ndm, out_ld), dtype=torch.float32, device=data.device)
        code = torch.empty((ndm, out_ld), dtype=torch.int32, device=data.device)
        if spectrum is not None:
            spec_all = spectrum
            if spec_all.dtype != torch.complex64 or not spec_all.is_contiguous():
                spec_all = spec_all.to(torch.complex64).contiguous()
        L = _lib.lib()
        step = ndm if spectrum is not None else p["chunk"]
        wplan = p["whiten"]
        if wplan is not None:
            edges_d, zap_d = self._whiten_tables(wplan, p["zap"], data.device)
            med = torch.empty((step, wplan.nblk), dtype=torch.float32, device=data.device)
            scale32 = torch.ones(ndm, dtype=torch.float32, device=data.device)
        # 8 and 16 harmonics: the kernel's power pass (half a spectrum chunk of workspace); below, gathering
        # from the spectrum itself is as fast or faster -- the same bits either way
        work = torch.empty(step * nbin, dtype=torch.float32, device=data.device) if p["nl"] > 3 else None
        for lo in range(0, ndm, step):
            hi = min(ndm, lo + step)
            spec = spec_all if spectrum is not None else self._spectrum_rows(data, mean32, lo, hi, p["n_used"],
                                                                             p["nfft"])
            if wplan is not None:
                # (the caller's own tensor is left alone; a converted copy of it is ours)
                spec = self._whiten_rows(L, spec, nbin, wplan, edges_d, zap_d, med,
                                         torch.empty_like(spec) if spec is spectrum else None)
            rc = L.pss_harmonic_search(_engine.ptr(spec), hi - lo, nbin, int(spec.shape[1]),
                                       _engine.ptr(scale32[lo:hi]), p["nl"], p["kmin"], ce, _engine.ptr(snr[lo:hi]),
                                       _engine.ptr(code[lo:hi]), out_ld, _engine.ptr(work), _engine.stream_ptr())
            _lib.check(rc, "harmonic_search")
            del spec
        snr, code = snr[:, :nq], code[:, :nq]
        k, lev, freq = self._decode_cells(code, ce, p["df"])
        cells = HarmonicPlane(snr, k, lev, code, freq, p["df"], p["nfft"], nbin, p["kmin"], ce, mean_d, std_d, plane)
        if wplan is not None:
            cells.whiten = wplan
        return cells

    def periodicity_search(self, plane, threshold=10.0, nharm=16, cell=32, dm_tol=1, freq_tol=1.0,
                           max_cells=1 << 20, nfft=None, fmin=None, mean=None, std=None, stat_block=1024,
                           max_bytes=1 << 30, spectrum=None, whiten=None, zap=None):
        """Periodicity search of a DM-time plane (extension: the reference has
        no counterpart): :meth:`harmonic_snr`, then the cells with
        ``snr >= threshold`` -- found on the device, only they cross to the
        host -- clustered friends-of-friends into candidates.

        Cells a and b (trial j, fundamental f = bin / 2^l bins) are friends iff
        ``|j_a - j_b| <= dm_tol`` and ``|f_a - f_b| <= freq_tol`` bins (compared
        exactly, in sixteenths of a bin); a cluster is a connected component and
        its candidate the cell that is the lexicographic maximum of (snr,
        -dm_index, -bin).  Harmonically related candidates (f, 2 f, f / 2 ...)
        stay separate: sifting them is left to the caller.  More than
        ``max_cells`` cells above the threshold raise ValueError.

        ``snr`` is the sum in units of its own standard deviation, but the sum
        of a few exponential powers is not Gaussian: in white noise one bin
        reaches z = 10 at h = 1 with probability e^-11, where a Gaussian would
        give 8e-24.  Hence the default threshold above the single-pulse
        search's, and ``log_fap``, the logarithm of the single-trial
        false-alarm probability of each candidate from the chi-square
        distribution with 2 h degrees of freedom; multiply the probability by
        the number of (trial, bin, level) searched.  ``whiten`` / ``zap`` are
        those of :meth:`harmonic_snr`: on data with red noise or interference
        lines the unwhitened search returns little else.  Returns
        :class:`PeriodCandidates`."""
        p = self._harmonic_plan(plane, nharm, cell, nfft, fmin, threshold, dm_tol, freq_tol, max_cells, mean, std,
                                stat_block, max_bytes, spectrum, whiten, zap)
        cells = self.harmonic_snr(plane, nharm=nharm, cell=cell, nfft=nfft, fmin=fmin, mean=mean, std=std,
                                  stat_block=stat_block, max_bytes=max_bytes, spectrum=spectrum, whiten=whiten,
                                  zap=zap)
        return PeriodCandidates(self._period_cells("periodicity_search", plane, cells, p)[0], cells, p["threshold"])

    def _period_cells(self, what, plane, cells, p, *maps):
        """The cells above the threshold of the plan ``p``, clustered on (trial, fundamental): (the array of
        :func:`period_candidates_from_cells`, packed int64: trial, bin, level, then ``maps`` at every such cell)."""
        s, packed = self._cells_above(what, cells, p["threshold"], p["max_cells"], cells.bin, cells.nharm_log2, *maps)
        return period_candidates_from_cells(s, packed[0], packed[1], packed[2], plane.dms, cells.df, p["dm_tol"],
                                            p["freq_tol"]), packed
