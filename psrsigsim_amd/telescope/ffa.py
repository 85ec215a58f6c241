"""Fast folding search: the plane's series folded coherently at every period they resolve, octave by octave,
their profiles matched with circular boxcars, thresholded and clustered."""
import math

import numpy as np
import torch

from .._units import to_value
from .. import _engine, _lib
from .plane import (PlaneStage, cluster_cells, _cluster_candidates, _check_plane, _integers, _check_cells, _threshold,
                    _given_stats)
from .periodicity import PeriodCandidates


class FFAPlane(object):
    """Result of :meth:`Backend.ffa_snr`: the best boxcar of every cell of
    ``cell`` consecutive folded profiles of every trial, on the device.  The
    columns are every (octave, base period, cell) in plan order -- the table
    ``columns``.

    ``snr``        torch float32 [nDM, ncols], -inf where a cell holds no candidate
    ``code``       torch int32 [nDM, ncols], the kernel's (k << 16) | (s - q * cell)
    ``phase``      torch int32 [nDM, ncols], first bin of the winning box
    ``shift``      torch int64 [nDM, ncols], the winning profile s of its base period
    ``width_log2`` torch int32 [nDM, ncols], the box is 2**width_log2 bins wide
    ``period``     torch float64 [nDM, ncols], the winner's period in seconds,
                   (p + s / (m - 1)) * 2^lf / fs
    ``columns``    host int64 [ncols, 5]: octave, lf, p (base period in
                   scrunched samples), m (rows folded, n // p) and q (the cell)
    ``mean``       torch float64 [nDM], the baseline subtracted from each trial
    ``std``        torch float64 [nDM], the noise of one sample of each trial
                   (0: a trial without a usable variance, its S/N is 0)
    ``cell``       profiles per cell
    ``plan``       the octaves (:meth:`Backend.ffa_plan`)
    ``plane``      the :class:`DedispersedPlane` that was searched"""

    def __init__(self, snr, code, phase, shift, width_log2, period, columns, mean, std, cell, plan, plane):
        self.snr = snr
        self.code = code
        self.phase = phase
        self.shift = shift
        self.width_log2 = width_log2
        self.period = period
        self.columns = columns
        self.mean = mean
        self.std = std
        self.cell = cell
        self.plan = plan
        self.plane = plane

    def __repr__(self):
        return "FFAPlane(%d trials x %d cells of %d profiles, %d octaves)" % (
            self.snr.shape[0], self.snr.shape[1], self.cell, len(self.plan))


FFA_DTYPE = np.dtype([("snr", np.float32), ("dm_index", np.int32), ("dm", np.float64), ("period", np.float64),
                      ("freq", np.float64), ("width", np.int64), ("width_sec", np.float64), ("phase", np.int64),
                      ("bins", np.int64), ("octave", np.int32), ("shift", np.int64), ("ncells", np.int64)])


class FFACandidates(PeriodCandidates):
    """Result of :meth:`Backend.ffa_search`: one candidate per cluster of cells
    above the threshold, on the host, ordered by ``snr`` descending, then
    (``dm_index``, ``period``) ascending.  A :class:`PeriodCandidates`, so
    :meth:`Backend.fold_candidates` takes it as it stands.

    ``array`` is the NumPy structured array (``FFA_DTYPE``); every field is also
    an attribute: ``snr``, ``dm_index``, ``dm`` (pc/cm^3), ``period`` (s),
    ``freq`` (Hz), ``width`` (bins of the scrunched series), ``width_sec``,
    ``phase`` (first bin of the box), ``bins`` (the base period p in scrunched
    samples), ``octave``, ``shift`` (the profile s) and ``ncells`` (cells of the
    cluster).  ``cells`` is the :class:`FFAPlane` and ``threshold`` the cut."""
    _dtype = FFA_DTYPE


def ffa_candidates_from_cells(snr, dm_index, column, shift, width_log2, phase, columns, T, fs, dms, dm_tol=1,
                              freq_tol=1.0):
    """Cluster the cells (``dm_index``, fundamental F) with
    :func:`cluster_cells` -- F = round(16 T / P) for a period of P samples of
    the raw series, the fundamental in sixteenths of a Fourier bin (the key of
    :func:`period_candidates_from_cells`), width 0 and a tolerance of
    round(16 freq_tol) -- and return the structured array of one candidate per
    cluster, its lexicographic maximum of (snr, -dm_index, -F), in the order of
    :class:`FFACandidates`.  ``column`` indexes the table ``columns`` of the
    :class:`FFAPlane`."""
    snr = np.asarray(snr, dtype=np.float32)
    j = np.asarray(dm_index, dtype=np.int64)
    col = np.asarray(columns, dtype=np.int64).reshape(-1, 5)[np.asarray(column, dtype=np.int64)]
    s = np.asarray(shift, dtype=np.int64)
    octave, lf, p, m = col[:, 0], col[:, 1], col[:, 2], col[:, 3]
    scale = np.ldexp(1.0, lf)
    period = (p + s.astype(np.float64) / (m - 1)) * scale / float(fs)
    F = np.rint(16.0 * T / (period * float(fs))).astype(np.int64)
    labels = cluster_cells(j, F, np.zeros_like(F), dm_tol, int(round(16 * float(freq_tol))))
    out, best = _cluster_candidates(FFA_DTYPE, labels, snr, j, F, dms)
    out["period"] = period[best]
    with np.errstate(divide="ignore"):
        out["freq"] = 1.0 / out["period"]
    out["width"] = np.left_shift(1, np.asarray(width_log2, dtype=np.int64)[best])
    out["width_sec"] = out["width"] * scale[best] / float(fs)
    out["phase"] = np.asarray(phase, dtype=np.int64)[best]
    out["bins"] = p[best]
    out["octave"] = octave[best]
    out["shift"] = s[best]
    final = np.lexsort((out["period"], out["dm_index"], -out["snr"].astype(np.float64)))
    return out[final]


class FFAStage(PlaneStage):
    @staticmethod
    def ffa_plan(T, samprate, pmin, pmax, bins=256):
        """The octave plan of the fast folding search of series of ``T``
        samples at ``samprate`` (MHz, as ``DedispersedPlane.samprate``) for the
        periods ``pmin`` .. ``pmax`` (s), on the host.  With fs the rate in Hz,
        a = pmin fs, b = pmax fs samples and B = ``bins`` (an integer in [16,
        2048]), B <= a <= b: octave lf scrunches the series by 2^lf to
        n = T >> lf samples and folds it at the base periods p0 .. p0 + np - 1
        scrunched samples -- every profile has between B and 2 B - 1 bins.  The
        octaves run lf = floor(log2(a / B)), lf + 1 .. while B 2^lf <= b; p0 is
        B, in the first octave max(B, floor(a / 2^lf)), and the last period
        min(2 B - 1, ceil(b / 2^lf)).  Every period must fold at least two rows
        (floor(n / p) >= 2) and lf stay within 16.  Returns the list of octaves,
        dicts of ``lf``, ``n``, ``p0``, ``np`` and the range ``pmin``, ``pmax``
        in seconds the octave's profiles cover."""
        what = "ffa_plan"
        T, B = _integers(what, "T and bins", T, bins)
        if B < 16 or B > 2048:
            raise ValueError("%s: bins %d outside [16, 2048]" % (what, B))
        try:
            fs = float(to_value(samprate, 'MHz')) * 1e6
            a, b = float(to_value(pmin, 's')) * fs, float(to_value(pmax, 's')) * fs
        except (TypeError, ValueError):
            fs = a = b = np.nan
        if not (np.isfinite(fs) and fs > 0 and np.isfinite(a) and np.isfinite(b)):
            raise ValueError("%s: samprate %r, pmin %r and pmax %r are not finite" % (what, samprate, pmin, pmax))
        if not (B <= a <= b):
            raise ValueError("%s: pmin (%.6g samples) and pmax (%.6g samples) do not satisfy bins %d <= pmin <= pmax"
                             % (what, a, b, B))
        lf = int(math.floor(math.log2(a / B)))
        while B * 2.0 ** (lf + 1) <= a:                        # (the logarithm's rounding, either way)
            lf += 1
        while B * 2.0 ** lf > a:
            lf -= 1
        first = lf
        plan = []
        while B * 2.0 ** lf <= b:
            if lf > 16:
                raise ValueError("%s: pmax needs a scrunch by 2^%d, beyond 2^16 -- raise bins" % (what, lf))
            n = T >> lf
            p0 = max(B, int(math.floor(a / 2.0 ** lf))) if lf == first else B
            pl = min(2 * B - 1, int(math.ceil(b / 2.0 ** lf)))
            if n // pl < 2:
                raise ValueError("%s: %d samples scrunched by 2^%d hold fewer than two periods of %d bins"
                                 % (what, T, lf, pl))
            plan.append(dict(lf=lf, n=n, p0=p0, np=pl - p0 + 1, pmin=p0 * 2.0 ** lf / fs,
                             pmax=(pl + 1) * 2.0 ** lf / fs))
            lf += 1
        return plan

    @staticmethod
    def _ffa_plan(plane, pmin, pmax, bins=256, nwidths=6, cell=16, threshold=8.0, dm_tol=1, freq_tol=1.0,
                  max_cells=1 << 20, mean=None, std=None, stat_block=1024, max_bytes=1 << 30):
        """Validate the arguments of :meth:`ffa_snr` and :meth:`ffa_search` on
        the host (nothing touches the device): a dict of ndm, T, fs (Hz), plan,
        nw, cell, threshold, dm_tol, freq_tol, max_cells, mean, std (float64
        [nDM] or None), stat_block and max_bytes."""
        what = "ffa search"
        ndm, T = _check_plane(what, plane, 4, "too small")
        nw, ce, sb, mc, mb = _integers(what, "nwidths, cell, stat_block, max_cells and max_bytes", nwidths, cell,
                                       stat_block, max_cells, max_bytes)
        if nw < 1 or nw > 11:
            raise ValueError("%s: nwidths %d outside [1, 11]" % (what, nw))
        _check_cells(what, ce, sb, mc)
        plan = FFAStage.ffa_plan(T, plane.samprate, pmin, pmax, bins)
        if mb < 8 * plan[0]["n"]:
            raise ValueError("%s: max_bytes %d is below the two buffers of one trial and period (%d bytes)"
                             % (what, mb, 8 * plan[0]["n"]))
        th = _threshold(what, threshold, dm_tol, "freq_tol", freq_tol)
        mean, std = _given_stats(what, mean, std, ndm)
        return dict(ndm=ndm, T=T, fs=float(to_value(plane.samprate, 'MHz')) * 1e6, plan=plan, nw=nw, cell=ce,
                    threshold=th, dm_tol=dm_tol, freq_tol=freq_tol, max_cells=mc, mean=mean, std=std, stat_block=sb,
                    max_bytes=mb)

    @staticmethod
    def _ffa_chunks(ndm, n, npd, max_bytes):
        """The (trial lo, hi, period lo, hi) chunks of one octave whose two buffers of hi - lo trials x periods
        x n floats stay within ``max_bytes``: whole trials where one fits, else one trial's periods in runs."""
        per = 8 * n
        trials = max_bytes // (per * npd)
        if trials >= 1:
            return [(lo, min(ndm, lo + trials), 0, npd) for lo in range(0, ndm, trials)]
        run = max(1, max_bytes // per)
        return [(i, i + 1, lo, min(npd, lo + run)) for i in range(ndm) for lo in range(0, npd, run)]

    def ffa_snr(self, plane, pmin, pmax, bins=256, nwidths=6, cell=16, mean=None, std=None, stat_block=1024,
                max_bytes=1 << 30):
        """Fast folding search of a DM-time plane on the device (extension:
        the reference has no counterpart): the time-domain complement of
        :meth:`harmonic_snr` for long periods and small duty cycles.  Per
        octave of :meth:`ffa_plan` (``pmin``, ``pmax`` in seconds, ``bins``)
        every trial is scrunched by 2^lf with its float32 mean subtracted
        (``pss_ffa_scrunch``), folded at every base period p by the fast
        folding transform (``pss_ffa_transform``: m = n // p rows give the m
        profiles at the periods p + s / (m - 1), s < m, in ceil(log2 m) levels
        of adds), and every profile searched with circular boxcars of 2^k bins,
        k < ``nwidths``, 2^(k+1) <= p (``pss_ffa_profile_search``):

            z = (sum of the box) * 2^(-k/2) / (std sqrt(m 2^lf))

        in float32 in the fixed order of include/pss_hip.h.  Per cell of
        ``cell`` (a power of two in [16, 2048]) consecutive profiles the
        largest z is kept -- ties to the narrower box, then the lower shift,
        then the lower phase.  Returns an :class:`FFAPlane`.

        z is the box sum over the noise of the box, on a series whose baseline
        is the subtracted mean: there is no off-pulse (w / p) term, so a pulse
        that fills much of its period is underrated.

        ``mean`` / ``std`` are as in :meth:`boxcar_snr`: given, or the block
        medians measured on the device; a trial whose variance is not positive
        and finite gets S/N 0.  The transform runs in chunks of (trials x base
        periods) whose two buffers stay within ``max_bytes``; the maps do not
        depend on the chunking.  No host synchronisation."""
        p = self._ffa_plan(plane, pmin, pmax, bins=bins, nwidths=nwidths, cell=cell, mean=mean, std=std,
                           stat_block=stat_block, max_bytes=max_bytes)
        ndm, T, ce, nw, fs = p["ndm"], p["T"], p["cell"], p["nw"], p["fs"]
        data, ld = self._plane_rows(plane.data)
        dev = data.device
        if p["mean"] is not None:
            mean32 = _engine.to_dev(p["mean"].astype(np.float32))
            rstd32 = _engine.to_dev((1.0 / p["std"]).astype(np.float32))
            mean_d, std_d = _engine.to_dev(p["mean"]), _engine.to_dev(p["std"])
        else:
            mean_d, var = self._trial_stats(data, ld, p["stat_block"])
            good = torch.isfinite(var) & (var > 0)
            std_d = torch.where(good, torch.sqrt(var), torch.zeros_like(var))
            mean32 = mean_d.to(torch.float32)
            rstd32 = torch.where(good, 1.0 / torch.sqrt(var), torch.zeros_like(var)).to(torch.float32)
        L = _lib.lib()
        snrs, codes, phases, cols = [], [], [], []
        for o, oc in enumerate(p["plan"]):
            lf, n, p0, npd = oc["lf"], oc["n"], oc["p0"], oc["np"]
            y_ld = (n + 3) // 4 * 4
            y = torch.empty((ndm, y_ld), dtype=torch.float32, device=dev)
            _lib.check(L.pss_ffa_scrunch(_engine.ptr(data), ndm, T, ld, _engine.ptr(mean32), lf, _engine.ptr(y), y_ld,
                                         _engine.stream_ptr()), "ffa_scrunch")
            ms = [n // (p0 + pi) for pi in range(npd)]
            rm = _engine.to_dev(np.array([1.0 / math.sqrt(m * 2.0 ** lf) for m in ms]).astype(np.float32))
            nq = (ms[0] + ce - 1) // ce
            snr = torch.empty((ndm, npd, nq), dtype=torch.float32, device=dev)
            code = torch.empty((ndm, npd, nq), dtype=torch.int32, device=dev)
            phase = torch.empty((ndm, npd, nq), dtype=torch.int32, device=dev)
            chunks = self._ffa_chunks(ndm, n, npd, p["max_bytes"])
            words = max((hi - lo) * (pb - pa) for lo, hi, pa, pb in chunks) * n
            buf = torch.empty((2, words), dtype=torch.float32, device=dev)
            for lo, hi, pa, pb in chunks:
                _lib.check(L.pss_ffa_transform(_engine.ptr(y[lo:hi]), hi - lo, n, y_ld, p0 + pa, pb - pa,
                                               _engine.ptr(buf[0]), _engine.ptr(buf[1]), _engine.stream_ptr()),
                           "ffa_transform")
                # (a chunk is whole trials of every period, or periods pa .. pb of one trial: rows of nq either way)
                _lib.check(L.pss_ffa_profile_search(_engine.ptr(buf[0]), hi - lo, n, p0 + pa, pb - pa,
                                                    _engine.ptr(rstd32[lo:hi]), _engine.ptr(rm[pa:pb]), nw, ce,
                                                    _engine.ptr(snr[lo:hi, pa:pb]), _engine.ptr(code[lo:hi, pa:pb]),
                                                    _engine.ptr(phase[lo:hi, pa:pb]), nq, _engine.stream_ptr()),
                           "ffa_profile_search")
            del buf, y
            # the cells a period has (the kernel pads every period's row to the nq of the shortest)
            keep = np.concatenate([pi * nq + np.arange((m + ce - 1) // ce) for pi, m in enumerate(ms)])
            cols.append(np.stack([np.full(keep.size, o), np.full(keep.size, lf), p0 + keep // nq,
                                  np.asarray(ms, dtype=np.int64)[keep // nq], keep % nq], axis=1).astype(np.int64))
            keep_d = _engine.to_dev(keep.astype(np.int64))
            _engine.wait_uploads()
            snrs.append(snr.view(ndm, npd * nq).index_select(1, keep_d))
            codes.append(code.view(ndm, npd * nq).index_select(1, keep_d))
            phases.append(phase.view(ndm, npd * nq).index_select(1, keep_d))
        columns = np.concatenate(cols, axis=0)
        snr, code, phase = torch.cat(snrs, dim=1), torch.cat(codes, dim=1), torch.cat(phases, dim=1)
        # the winner's shift and period from the column table (float64, the operations of the docstring in order)
        tab = _engine.to_dev(np.stack([columns[:, 2], columns[:, 3] - 1, np.ldexp(1.0, columns[:, 1]),
                                       columns[:, 4] * float(ce), np.full(columns.shape[0], fs)]).astype(np.float64))
        _engine.wait_uploads()
        shift = tab[3].to(torch.int64)[None, :] + (code & 0xFFFF).to(torch.int64)
        # (a tensor divisor: torch divides by a Python scalar as a product with its reciprocal)
        period = (tab[0][None, :] + shift.to(torch.float64) / tab[1][None, :]) * tab[2][None, :] / tab[4][None, :]
        return FFAPlane(snr, code, phase, shift, code >> 16, period, columns, mean_d, std_d, ce, p["plan"], plane)

    def ffa_search(self, plane, pmin, pmax, threshold=8.0, bins=256, nwidths=6, cell=16, dm_tol=1, freq_tol=1.0,
                   max_cells=1 << 20, mean=None, std=None, stat_block=1024, max_bytes=1 << 30):
        """Fast folding search of a DM-time plane (extension: the reference
        has no counterpart): :meth:`ffa_snr`, then the cells with
        ``snr >= threshold`` -- found on the device, only they cross to the
        host -- clustered friends-of-friends into candidates.

        Cells a and b (trial j, period P samples of the raw series) are friends
        iff ``|j_a - j_b| <= dm_tol`` and their fundamentals T / P differ by at
        most ``freq_tol`` Fourier bins of the raw series (compared in
        sixteenths of a bin, F = round(16 T / P), the key of
        :meth:`periodicity_search`); a cluster is a connected component and its
        candidate the cell that is the lexicographic maximum of (snr,
        -dm_index, -F).  More than ``max_cells`` cells above the threshold
        raise ValueError.

        z is the box sum over the noise of the box on a series whose baseline
        is the subtracted mean -- no off-pulse (w / p) term -- and Gaussian in
        white noise, hence a threshold near the single-pulse search's.
        Harmonically related candidates (P, 2 P, P / 2 ...) stay separate:
        sifting them is left to the caller.  Returns :class:`FFACandidates`."""
        p = self._ffa_plan(plane, pmin, pmax, bins, nwidths, cell, threshold, dm_tol, freq_tol, max_cells, mean, std,
                           stat_block, max_bytes)
        cells = self.ffa_snr(plane, pmin, pmax, bins=bins, nwidths=nwidths, cell=cell, mean=mean, std=std,
                             stat_block=stat_block, max_bytes=max_bytes)
        ncols = int(cells.snr.shape[1])
        column = torch.arange(ncols, dtype=torch.int64, device=cells.snr.device)[None, :].expand(p["ndm"], ncols)
        s, packed = self._cells_above("ffa_search", cells, p["threshold"], p["max_cells"], column, cells.shift,
                                      cells.width_log2, cells.phase)
        arr = ffa_candidates_from_cells(s, packed[0], packed[1], packed[2], packed[3], packed[4], cells.columns,
                                        p["T"], p["fs"], plane.dms, p["dm_tol"], p["freq_tol"])
        return FFACandidates(arr, cells, p["threshold"])
