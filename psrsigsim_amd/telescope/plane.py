"""Shared by the stages that search a DM-time plane: the plane, the argument checks (``what`` is the message
prefix), the candidate container, the clustering and, in :class:`PlaneStage` (the stages' base), the device steps."""
import numpy as np
import torch

from .. import _engine, _lib


class DedispersedPlane(object):
    """Result of :meth:`Backend.dedisperse`: the DM-time plane on the device.

    ``data``      torch float32 [nDM, T] (T = N - max_delay), row j the sum over
                  the channels of the signal shifted by ``delays[j]``
    ``dms``       the trial DMs, float64 [nDM] (pc/cm^3)
    ``delays``    the host table, int32 [nDM][C_local] samples
    ``samprate``  sample rate of the series, MHz
    ``ref_freq``  the frequency the delays refer to, MHz
    ``max_delay`` the table's maximum, samples
    ``subband``   None, or the :class:`SubbandPlan` of a plane that :meth:`Backend.subband_dedisperse` made
                  (``delays`` is then its effective table)"""
    subband = None

    def __init__(self, data, dms, delays, samprate, ref_freq, max_delay):
        self.data = data
        self.dms = dms
        self.delays = delays
        self.samprate = samprate
        self.ref_freq = ref_freq
        self.max_delay = max_delay

    def __repr__(self):
        return "DedispersedPlane(%d trials x %d samples, ref %.6g MHz)" % (
            self.data.shape[0], self.data.shape[1], self.ref_freq)


class Candidates(object):
    """One candidate per cluster of cells above the threshold, on the host: ``array`` (structured, the
    subclass's ``_dtype``; every field also an attribute), ``cells`` (the map searched) and ``threshold``."""
    _dtype, _above = np.dtype([]), "above"

    def __init__(self, array, cells, threshold):
        self.array = array
        self.cells = cells
        self.threshold = threshold

    def __len__(self):
        return len(self.array)

    def __getitem__(self, i):
        return self.array[i]

    def __getattr__(self, name):
        if name != "array" and name in self._dtype.names:
            return self.array[name]
        raise AttributeError(name)

    def __repr__(self):
        return "%s(%d %s %g)" % (type(self).__name__, len(self.array), self._above, self.threshold)


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _check_plane(what, plane, tmin=None, size=None):
    """(nDM, T) of a :class:`DedispersedPlane`; ValueError for anything else, and (given ``tmin``) for a
    plane without a trial or with fewer samples: "the plane is ``size``"."""
    if not isinstance(plane, DedispersedPlane):
        raise ValueError("%s takes a DedispersedPlane, not %s" % (what, type(plane).__name__))
    ndm, T = int(plane.data.shape[0]), int(plane.data.shape[1])
    if tmin is not None and (ndm < 1 or T < tmin):
        raise ValueError("%s: the plane is %s (%d trials x %d samples)" % (what, size, ndm, T))
    return ndm, T


def _integers(what, names, *values):
    """``values`` as ints; ValueError ("``names`` are integers") unless every one is a whole number."""
    try:
        out = [int(v) for v in values]
        if all(o == v for o, v in zip(out, values)):
            return out
    except (TypeError, ValueError, OverflowError):
        pass
    raise ValueError("%s: %s are integers" % (what, names))


def _check_cells(what, cell, stat_block, max_cells):
    if cell < 16 or cell > 2048 or (cell & (cell - 1)):
        raise ValueError("%s: cell %d is not a power of two in [16, 2048]" % (what, cell))
    if stat_block < 2:
        raise ValueError("%s: stat_block %d < 2" % (what, stat_block))
    if max_cells < 0:
        raise ValueError("%s: max_cells %d < 0" % (what, max_cells))


def _threshold(what, threshold, dm_tol, tol_name, tol):     # (the tolerances: checked right after it in every plan)
    th = float(threshold)
    if not np.isfinite(th) or th <= 0:
        raise ValueError("%s: threshold %r is not finite and positive" % (what, threshold))
    if not (dm_tol >= 0) or not (tol >= 0):
        raise ValueError("%s: dm_tol %r and %s %r must not be negative" % (what, dm_tol, tol_name, tol))
    return th


def _given_stats(what, mean, std, ndm):
    """The user's ``mean`` / ``std`` as float64 [nDM] each (scalars repeated), or (None, None)."""
    if (mean is None) != (std is None):
        raise ValueError("%s: give both mean and std, or neither" % what)
    if mean is None:
        return None, None
    stats = []
    for name, v in (("mean", mean), ("std", std)):
        a = np.asarray(v, dtype=np.float64)
        if a.ndim == 0:
            a = np.full(ndm, float(a))
        if a.ndim != 1 or a.size != ndm:
            raise ValueError("%s: %s has %s entries for %d trials"
                             % (what, name, "x".join(str(s) for s in a.shape), ndm))
        if not np.all(np.isfinite(a)):
            raise ValueError("%s: %s has an entry that is not finite" % (what, name))
        stats.append(a)
    mean, std = stats
    if np.any(std <= 0):
        raise ValueError("%s: std has an entry <= 0" % what)
    return mean, std


def cluster_cells(dm_index, time, width, dm_tol=1, time_tol=0):
    """Friends-of-friends labels of the cells (``dm_index``, box ``[time,
    time + width)``): a and b are friends iff ``|j_a - j_b| <= dm_tol`` and
    ``max(t_a, t_b) - min(t_a + w_a, t_b + w_b) <= time_tol`` (at 0: boxes that
    overlap or touch); clusters are the connected components.  Returns int64
    labels, the smallest cell index of each cluster.

    Sort-and-sweep with union-find, O(n (2 dm_tol + 1)): the cells are taken by
    rising start time.  A later cell b is a friend of an earlier cell a of trial
    j' iff ``t_b <= t_a + w_a + time_tol``, so of some cell of j' iff t_b is
    within the trial's furthest reach so far -- and then of the cell a* that
    reaches furthest, to which every other friend of b in j' is itself a friend
    (both start by t_b and reach it).  Linking b to a* of each trial within
    dm_tol therefore joins the same components as testing all pairs."""
    j = np.asarray(dm_index, dtype=np.int64)
    t = np.asarray(time, dtype=np.int64)
    w = np.asarray(width, dtype=np.int64)
    n = j.size
    parent = list(range(n))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r

    reach = {}                                      # trial -> (furthest end + tol so far, its cell)
    order = np.argsort(t, kind="stable")
    jl, tl, el = j.tolist(), t.tolist(), (t + w + int(time_tol)).tolist()
    dmt = int(dm_tol)
    for b in order.tolist():
        jb, tb = jl[b], tl[b]
        for jj in range(jb - dmt, jb + dmt + 1):
            r = reach.get(jj)
            if r is not None and tb <= r[0]:
                ra, rb = find(r[1]), find(b)
                if ra != rb:
                    if ra < rb:
                        parent[rb] = ra
                    else:
                        parent[ra] = rb
        r = reach.get(jb)
        if r is None or el[b] > r[0]:
            reach[jb] = (el[b], b)
    return np.array([find(a) for a in range(n)], dtype=np.int64)


def _cluster_candidates(dtype, labels, snr, j, t, dms):
    """(out, best): a row of ``dtype`` per cluster with the ``snr``, ``dm_index`` and ``dm`` of its best cell
    (snr descending, then ``j``, ``t`` ascending) and its ``ncells``; and the index of that cell."""
    order = np.lexsort((t, j, -snr.astype(np.float64), labels))
    lab = labels[order]
    first = np.ones(lab.size, dtype=bool)
    first[1:] = lab[1:] != lab[:-1]
    best = order[first]
    out = np.empty(best.size, dtype=dtype)
    out["snr"] = snr[best]
    out["dm_index"] = j[best]
    out["dm"] = np.asarray(dms, dtype=np.float64)[j[best]] if best.size else 0.0
    out["ncells"] = np.diff(np.append(np.flatnonzero(first), lab.size))
    return out, best


class PlaneStage(object):
    @staticmethod
    def _plane_rows(data):
        if data.dtype != torch.float32 or data.stride(1) != 1:
            data = data.to(torch.float32).contiguous()
        return data, _engine.row_stride(data)

    @staticmethod
    def _trial_stats(data, ld, stat_block):
        """Robust per-trial statistics on the device, no host synchronisation:
        ``pss_chan_stats`` over whole blocks of sb = min(stat_block, T) samples
        (trailing samples do not enter), per block m = sum / sb and
        v = sumsq / sb - m^2 in float64, and per trial the lower median (sorted
        index (nb - 1) // 2) of each over its nb blocks -- a block that holds a
        pulse does not move a median.  Returns (mean, var) float64 [nDM]."""
        ndm, T = int(data.shape[0]), int(data.shape[1])
        sb = min(int(stat_block), T)
        nb = T // sb
        s1 = torch.empty((nb, ndm), dtype=torch.float64, device=data.device)
        s2 = torch.empty_like(s1)
        mn = torch.empty((nb, ndm), dtype=torch.float32, device=data.device)
        mx = torch.empty_like(mn)
        # (at most 65535 trials a call: pss_chan_stats says so beyond)
        _lib.check(_lib.lib().pss_chan_stats(_engine.ptr(data), ndm, ld, sb, nb, _engine.ptr(mn), _engine.ptr(mx),
                                             _engine.ptr(s1), _engine.ptr(s2), _engine.stream_ptr()), "chan_stats")
        m = s1 / sb
        v = s2 / sb - m * m
        mid = (nb - 1) // 2
        return torch.sort(m, dim=0).values[mid], torch.sort(v, dim=0).values[mid]

    @staticmethod
    def _cell_entries(code, cell):
        """A kernel's ``code`` [nDM, nq], level << 16 | entry - q cell, as (entry int64, level int32)."""
        q0 = torch.arange(code.shape[1], dtype=torch.int64, device=code.device) * cell
        return q0[None, :] + (code & 0xFFFF).to(torch.int64), code >> 16

    def _trial_mean(self, data, ld, ndm, mean, stat_block, what):
        """The per-trial baseline as a device float64 [nDM]: measured (block medians), a
        device tensor, or host values (uploaded, not yet fenced: ``_engine.wait_uploads``)."""
        if mean is None:
            return self._trial_stats(data, ld, stat_block)[0]
        if isinstance(mean, torch.Tensor):
            mean_d = mean.to(device=data.device, dtype=torch.float64)
        else:
            m = np.asarray(mean, dtype=np.float64)
            m = np.full(ndm, float(m)) if m.ndim == 0 else m
            if m.ndim != 1 or m.size != ndm or not np.all(np.isfinite(m)):
                raise ValueError("%s: mean must hold %d finite entries" % (what, ndm))
            mean_d = _engine.to_dev(m)
        if tuple(mean_d.shape) != (ndm,):
            raise ValueError("%s: mean has the shape %s for %d trials" % (what, tuple(mean_d.shape), ndm))
        return mean_d

    @staticmethod
    def _cells_above(what, cells, th, max_cells, *maps):
        """The cells with ``cells.snr >= th``, found on the device; only they cross to the host: (snr [n],
        packed int64 [1 + len(maps)][n]: the trial, then ``maps`` there).  ValueError beyond ``max_cells``."""
        idx = torch.nonzero(cells.snr >= th)
        n = int(idx.shape[0])
        if n > max_cells:
            raise ValueError("%s: %d cells at or above threshold %g exceed max_cells %d -- raise the threshold"
                             % (what, n, th, max_cells))
        j, q = idx[:, 0], idx[:, 1]
        packed = torch.stack((j,) + tuple(m[j, q].to(torch.int64) for m in maps)).cpu().numpy()
        return cells.snr[j, q].cpu().numpy(), packed
