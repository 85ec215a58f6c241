"""Single-pulse search: boxcar S/N of the DM-time plane, thresholded and clustered into candidates."""
import numpy as np
import torch

from .. import _engine, _lib
from .plane import (PlaneStage, Candidates, cluster_cells, _cluster_candidates, _check_plane, _integers, _check_cells,
                    _threshold, _given_stats)


class BoxcarPlane(object):
    """Result of :meth:`Backend.boxcar_snr`: the best boxcar of every cell of
    ``cell`` start times of every trial, on the device (nq = ceil(T / cell)).

    ``snr``        torch float32 [nDM, nq], -inf where a cell holds no candidate
    ``time``       torch int64 [nDM, nq], start sample of the winning box
    ``width_log2`` torch int32 [nDM, nq], its width is 2**width_log2 samples
    ``code``       torch int32 [nDM, nq], the kernel's (k << 16) | (t - q * cell)
    ``mean``       torch float64 [nDM], the baseline subtracted from each trial
    ``std``        torch float64 [nDM], the noise of one sample of each trial
                   (0: a trial without a usable variance, its S/N is 0)
    ``cell``       start times per cell
    ``plane``      the :class:`DedispersedPlane` that was searched"""

    def __init__(self, snr, time, width_log2, code, mean, std, cell, plane):
        self.snr = snr
        self.time = time
        self.width_log2 = width_log2
        self.code = code
        self.mean = mean
        self.std = std
        self.cell = cell
        self.plane = plane

    def __repr__(self):
        return "BoxcarPlane(%d trials x %d cells of %d samples)" % (self.snr.shape[0], self.snr.shape[1], self.cell)


CANDIDATE_DTYPE = np.dtype([("snr", np.float32), ("dm_index", np.int32), ("dm", np.float64), ("time", np.int64),
                            ("width", np.int64), ("t_sec", np.float64), ("ncells", np.int64)])


class PulseCandidates(Candidates):
    """Result of :meth:`Backend.single_pulse_search`: one candidate per cluster
    of cells above the threshold, on the host, ordered by ``snr`` descending,
    then (``dm_index``, ``time``, ``width``) ascending.

    ``array`` is the NumPy structured array (``CANDIDATE_DTYPE``); every field
    is also an attribute: ``snr``, ``dm_index``, ``dm`` (pc/cm^3), ``time``
    (start sample), ``width`` (samples), ``t_sec`` (the box centre in seconds
    at ``plane.ref_freq``) and ``ncells`` (cells of the cluster).  ``cells`` is
    the :class:`BoxcarPlane` and ``threshold`` the S/N cut."""
    _dtype = CANDIDATE_DTYPE
    _above = "above S/N"


def candidates_from_cells(snr, dm_index, time, width, dms, samprate_MHz, dm_tol=1, time_tol=0):
    """Cluster the cells (:func:`cluster_cells`) and return the structured
    array of one candidate per cluster -- its lexicographic maximum of
    (snr, -dm_index, -time) -- in the order of :class:`PulseCandidates`."""
    snr = np.asarray(snr, dtype=np.float32)
    j = np.asarray(dm_index, dtype=np.int64)
    t = np.asarray(time, dtype=np.int64)
    w = np.asarray(width, dtype=np.int64)
    labels = cluster_cells(j, t, w, dm_tol, time_tol)
    out, best = _cluster_candidates(CANDIDATE_DTYPE, labels, snr, j, t, dms)
    out["time"] = t[best]
    out["width"] = w[best]
    out["t_sec"] = (t[best] + w[best] / 2.0) / (float(samprate_MHz) * 1e6)
    final = np.lexsort((out["width"], out["time"], out["dm_index"], -out["snr"].astype(np.float64)))
    return out[final]


class PulseSearchStage(PlaneStage):
    @staticmethod
    def _search_plan(plane, nwidths=8, cell=32, threshold=6.0, dm_tol=1, time_tol=0, max_cells=1 << 20,
                     mean=None, std=None, stat_block=1024):
        """Validate the arguments of :meth:`boxcar_snr` and
        :meth:`single_pulse_search` on the host (nothing touches the device):
        returns (nDM, T, nwidths, cell, threshold, dm_tol, time_tol, max_cells,
        mean, std, stat_block), ``mean`` / ``std`` float64 [nDM] or None."""
        what = "single-pulse search"
        ndm, T = _check_plane(what, plane, 1, "empty")
        nw, ce, sb, mc = _integers(what, "nwidths, cell, stat_block and max_cells", nwidths, cell, stat_block,
                                   max_cells)
        if nw < 1 or nw > 13:
            raise ValueError("%s: nwidths %d outside [1, 13]" % (what, nw))
        _check_cells(what, ce, sb, mc)
        th = _threshold(what, threshold, dm_tol, "time_tol", time_tol)
        mean, std = _given_stats(what, mean, std, ndm)
        return ndm, T, nw, ce, th, dm_tol, time_tol, mc, mean, std, sb

    def boxcar_snr(self, plane, nwidths=8, cell=32, mean=None, std=None, stat_block=1024):
        """Boxcar matched filter of a DM-time plane on the device (extension:
        the reference has no counterpart).  For every trial j and every box
        [t, t + 2^k), k < ``nwidths``, inside the series,

            z = (sum of (plane[j] - mean[j]) over the box) * 2^(-k/2) / std[j]

        in float32 with the balanced summation tree of ``pss_boxcar_search``
        (include/pss_hip.h), and per cell of ``cell`` (a power of two in
        [16, 2048]) start times the largest z -- ties to the narrower box, then
        the earlier time.  One kernel reads the plane once; only the
        [nDM, ceil(T / cell)] map is written.  Returns a :class:`BoxcarPlane`.

        ``mean`` / ``std`` (both or neither; scalars or array-likes of length
        nDM) are the per-trial baseline and noise.  Left out, they are measured
        on the device (``pss_chan_stats`` and torch float64, no host
        synchronisation): the lower medians over blocks of ``stat_block``
        samples of the block means and block variances, which a block holding a
        pulse does not move (at most 65535 trials a call).  A trial whose
        variance is not positive and finite gets S/N 0 everywhere."""
        ndm, T, nw, ce, _, _, _, _, mean, std, sb = self._search_plan(
            plane, nwidths=nwidths, cell=cell, mean=mean, std=std, stat_block=stat_block)
        data, ld = self._plane_rows(plane.data)
        if mean is not None:
            mean32 = _engine.to_dev(mean.astype(np.float32))
            rstd32 = _engine.to_dev((1.0 / std).astype(np.float32))
            mean_d, std_d = _engine.to_dev(mean), _engine.to_dev(std)
        else:
            mean_d, var = self._trial_stats(data, ld, sb)
            good = torch.isfinite(var) & (var > 0)
            std_d = torch.where(good, torch.sqrt(var), torch.zeros_like(var))
            mean32 = mean_d.to(torch.float32)
            rstd32 = torch.where(good, 1.0 / torch.sqrt(var), torch.zeros_like(var)).to(torch.float32)
        nq = (T + ce - 1) // ce
        out_ld = (nq + 15) // 16 * 16                          # rows of whole 64-B segments
        snr = torch.empty((ndm, out_ld), dtype=torch.float32, device=data.device)[:, :nq]
        code = torch.empty((ndm, out_ld), dtype=torch.int32, device=data.device)[:, :nq]
        rc = _lib.lib().pss_boxcar_search(_engine.ptr(data), ndm, T, ld, _engine.ptr(mean32), _engine.ptr(rstd32),
                                          nw, ce, _engine.ptr(snr), _engine.ptr(code), out_ld,
                                          _engine.stream_ptr())
        _lib.check(rc, "boxcar_search")
        time, width_log2 = self._cell_entries(code, ce)
        return BoxcarPlane(snr, time, width_log2, code, mean_d, std_d, ce, plane)

    def single_pulse_search(self, plane, threshold=6.0, nwidths=8, cell=32, dm_tol=1, time_tol=0,
                            max_cells=1 << 20, mean=None, std=None, stat_block=1024):
        """Single-pulse search of a DM-time plane (extension: the reference has
        no counterpart): :meth:`boxcar_snr`, then the cells with
        ``snr >= threshold`` -- found on the device, only they cross to the
        host -- clustered friends-of-friends into candidates.

        Cells a and b (trial j, box [t, t + w)) are friends iff
        ``|j_a - j_b| <= dm_tol`` and ``max(t_a, t_b) - min(t_a + w_a,
        t_b + w_b) <= time_tol`` (at 0: boxes that overlap or touch); a cluster
        is a connected component and its candidate the cell that is the
        lexicographic maximum of (snr, -dm_index, -time).  More than
        ``max_cells`` cells above the threshold raise ValueError.  Returns
        :class:`PulseCandidates`."""
        _, _, nw, ce, th, dm_tol, time_tol, mc, mean, std, sb = self._search_plan(
            plane, nwidths, cell, threshold, dm_tol, time_tol, max_cells, mean, std, stat_block)
        cells = self.boxcar_snr(plane, nwidths=nw, cell=ce, mean=mean, std=std, stat_block=sb)
        s, packed = self._cells_above("single_pulse_search", cells, th, mc, cells.time, cells.width_log2)
        arr = candidates_from_cells(s, packed[0], packed[1], np.left_shift(1, packed[2]), plane.dms,
                                    plane.samprate, dm_tol, time_tol)
        return PulseCandidates(arr, cells, th)
