"""Backend -- mirrors ``psrsigsim/telescope/backend.py``."""
import numpy as np
import torch

from .._units import make_quant, to_value
from ..utils.constants import DM_K_VALUE
from .. import _engine, _lib

__all__ = ['Backend', 'DedispersedPlane', 'BoxcarPlane', 'PulseCandidates', 'HarmonicPlane', 'PeriodCandidates',
           'FoldedCandidates', 'AccelPlane', 'AccelCandidates']

C_M_S = 299792458.0                      # speed of light, m/s (exact)


class DedispersedPlane(object):
    """Result of :meth:`Backend.dedisperse`: the DM-time plane on the device.

    ``data``      torch float32 [nDM, T] (T = N - max_delay), row j the sum over
                  the channels of the signal shifted by ``delays[j]``
    ``dms``       the trial DMs, float64 [nDM] (pc/cm^3)
    ``delays``    the host table, int32 [nDM][C_local] samples
    ``samprate``  sample rate of the series, MHz
    ``ref_freq``  the frequency the delays refer to, MHz
    ``max_delay`` the table's maximum, samples"""

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


class PulseCandidates(object):
    """Result of :meth:`Backend.single_pulse_search`: one candidate per cluster
    of cells above the threshold, on the host, ordered by ``snr`` descending,
    then (``dm_index``, ``time``, ``width``) ascending.

    ``array`` is the NumPy structured array (``CANDIDATE_DTYPE``); every field
    is also an attribute: ``snr``, ``dm_index``, ``dm`` (pc/cm^3), ``time``
    (start sample), ``width`` (samples), ``t_sec`` (the box centre in seconds
    at ``plane.ref_freq``) and ``ncells`` (cells of the cluster).  ``cells`` is
    the :class:`BoxcarPlane` and ``threshold`` the S/N cut."""

    def __init__(self, array, cells, threshold):
        self.array = array
        self.cells = cells
        self.threshold = threshold

    def __len__(self):
        return len(self.array)

    def __getitem__(self, i):
        return self.array[i]

    def __getattr__(self, name):
        if name != "array" and name in CANDIDATE_DTYPE.names:
            return self.array[name]
        raise AttributeError(name)

    def __repr__(self):
        return "PulseCandidates(%d above S/N %g)" % (len(self.array), self.threshold)


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


def candidates_from_cells(snr, dm_index, time, width, dms, samprate_MHz, dm_tol=1, time_tol=0):
    """Cluster the cells (:func:`cluster_cells`) and return the structured
    array of one candidate per cluster -- its lexicographic maximum of
    (snr, -dm_index, -time) -- in the order of :class:`PulseCandidates`."""
    snr = np.asarray(snr, dtype=np.float32)
    j = np.asarray(dm_index, dtype=np.int64)
    t = np.asarray(time, dtype=np.int64)
    w = np.asarray(width, dtype=np.int64)
    labels = cluster_cells(j, t, w, dm_tol, time_tol)
    # best first within each label: snr descending, then dm_index, time ascending
    order = np.lexsort((t, j, -snr.astype(np.float64), labels))
    lab = labels[order]
    first = np.ones(lab.size, dtype=bool)
    first[1:] = lab[1:] != lab[:-1]
    best = order[first]
    count = np.diff(np.append(np.flatnonzero(first), lab.size))
    out = np.empty(best.size, dtype=CANDIDATE_DTYPE)
    out["snr"] = snr[best]
    out["dm_index"] = j[best]
    out["dm"] = np.asarray(dms, dtype=np.float64)[j[best]] if best.size else 0.0
    out["time"] = t[best]
    out["width"] = w[best]
    out["t_sec"] = (t[best] + w[best] / 2.0) / (float(samprate_MHz) * 1e6)
    out["ncells"] = count
    final = np.lexsort((out["width"], out["time"], out["dm_index"], -out["snr"].astype(np.float64)))
    return out[final]


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
    ``plane``      the :class:`DedispersedPlane` that was searched"""

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


class PeriodCandidates(object):
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

    def __init__(self, array, cells, threshold):
        self.array = array
        self.cells = cells
        self.threshold = threshold

    def __len__(self):
        return len(self.array)

    def __getitem__(self, i):
        return self.array[i]

    def __getattr__(self, name):
        if name != "array" and name in PERIOD_DTYPE.names:
            return self.array[name]
        raise AttributeError(name)

    def __repr__(self):
        return "PeriodCandidates(%d above %g)" % (len(self.array), self.threshold)


class AccelPlane(HarmonicPlane):
    """Result of :meth:`Backend.accel_snr`: per cell of every trial the best
    harmonic sum over the trial accelerations, on the device.  The fields of
    :class:`HarmonicPlane` (``snr``, ``bin``, ``nharm_log2``, ``code``,
    ``freq`` ... of the winning acceleration), and

    ``acc_index``  torch int32 [nDM, nq], the index into ``accels`` of the
                   acceleration that won the cell (the one given first on a
                   tie; 0 where ``snr`` is -inf)
    ``accels``     the trial accelerations, float64 [nacc] (m/s^2)"""

    def __init__(self, snr, bin, nharm_log2, code, freq, df, nfft, nbin, kmin, cell, mean, std, plane, acc_index,
                 accels):
        HarmonicPlane.__init__(self, snr, bin, nharm_log2, code, freq, df, nfft, nbin, kmin, cell, mean, std, plane)
        self.acc_index = acc_index
        self.accels = accels

    def __repr__(self):
        return "AccelPlane(%d trials x %d cells of %d bins, %d accelerations, df %.6g Hz)" % (
            self.snr.shape[0], self.snr.shape[1], self.cell, len(self.accels), self.df)


ACCEL_DTYPE = np.dtype(PERIOD_DTYPE.descr + [("accel", np.float64), ("acc_index", np.int32)])


class AccelCandidates(object):
    """Result of :meth:`Backend.accel_search`: the fields of
    :class:`PeriodCandidates` (same order, same meaning) plus ``accel`` (m/s^2)
    and ``acc_index``, the trial acceleration of the candidate's winning cell.
    ``array`` is the NumPy structured array (``ACCEL_DTYPE``), ``cells`` the
    :class:`AccelPlane` and ``threshold`` the cut."""

    def __init__(self, array, cells, threshold):
        self.array = array
        self.cells = cells
        self.threshold = threshold

    def __len__(self):
        return len(self.array)

    def __getitem__(self, i):
        return self.array[i]

    def __getattr__(self, name):
        if name != "array" and name in ACCEL_DTYPE.names:
            return self.array[name]
        raise AttributeError(name)

    def __repr__(self):
        return "AccelCandidates(%d above %g)" % (len(self.array), self.threshold)


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
    order = np.lexsort((k, j, -snr.astype(np.float64), labels))
    lab = labels[order]
    first = np.ones(lab.size, dtype=bool)
    first[1:] = lab[1:] != lab[:-1]
    best = order[first]
    count = np.diff(np.append(np.flatnonzero(first), lab.size))
    out = np.empty(best.size, dtype=PERIOD_DTYPE)
    out["snr"] = snr[best]
    out["dm_index"] = j[best]
    out["dm"] = np.asarray(dms, dtype=np.float64)[j[best]] if best.size else 0.0
    out["bin"] = k[best]
    out["nharm"] = np.left_shift(1, lev[best])
    out["freq"] = k[best] / np.left_shift(1, lev[best]).astype(np.float64) * float(df)
    with np.errstate(divide="ignore"):
        out["period"] = 1.0 / out["freq"]
    out["log_fap"] = harmonic_log_fap(out["snr"], out["nharm"]) if best.size else 0.0
    out["ncells"] = count
    final = np.lexsort((out["nharm"], out["bin"], out["dm_index"], -out["snr"].astype(np.float64)))
    return out[final]


def _host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def fold_chi2(p, H, M, V):
    """Reduced chi-square of a profile against a flat one (host, float64):
    ``sum over the bins with H_b > 0 of (p_b - M H_b)^2 / (V H_b) / (nbin - 1)``
    -- ``H`` the samples per bin, ``M`` / ``V`` the mean and variance of one
    sample.  0 when ``V`` is not positive and finite."""
    p = np.asarray(p, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64)
    if not (np.isfinite(V) and V > 0):
        return 0.0
    ok = H > 0
    d = p[ok] - M * H[ok]
    return float(np.sum(d * d / (V * H[ok])) / (p.size - 1))


def _fold_best(chis, n):
    """Index of the largest chi2 among the trials -n .. n (``chis[i + n]``):
    ties go to the smaller |i|, then to the smaller i."""
    best = 0
    for i in sorted(range(-n, n + 1), key=lambda v: (abs(v), v)):
        if chis[i + n] > chis[best + n]:
            best = i
    return best


class FoldedCandidates(object):
    """Result of :meth:`Backend.fold_candidates`: the phase x time x band cube
    of K periodicity candidates.

    ``cube``           torch float32 [K, nband, nsub, nbin] on the device: the
                       sub-band series of the candidate's DM folded at its
                       period (``pss_fold_series``)
    ``hits``           torch int32 [K, nsub, nbin], the samples per bin (the
                       same for every band)
    ``mean``, ``var``  torch float64 [K, nband], the block-median statistics of
                       one sample of each sub-band series
    ``dms``            float64 [K] (pc/cm^3)
    ``periods``        float64 [K] (s)
    ``period_samples`` float64 [K], Ps = period * samprate
    ``inc``            list of K Python ints, the phase step of one sample,
                       floor(2^64 / Ps + 1/2)
    ``band_w``         float64 [nband], the mean over the band's channels of
                       f_c^-2 - ref_freq^-2 (MHz^-2)
    ``samprate``       sample rate of the series, MHz
    ``ref_freq``       the frequency the delays refer to, MHz
    ``L``, ``T``       samples per sub-integration (T // nsub) and per series
    ``max_delay``      the delay table's maximum, samples"""

    def __init__(self, cube, hits, mean, var, dms, periods, period_samples, inc, band_w, samprate, ref_freq, L, T,
                 max_delay):
        self.cube = cube
        self.hits = hits
        self.mean = mean
        self.var = var
        self.dms = np.asarray(dms, dtype=np.float64)
        self.periods = np.asarray(periods, dtype=np.float64)
        self.period_samples = np.asarray(period_samples, dtype=np.float64)
        self.inc = [int(i) for i in inc]
        self.band_w = np.asarray(band_w, dtype=np.float64)
        self.samprate = samprate
        self.ref_freq = ref_freq
        self.L = int(L)
        self.T = int(T)
        self.max_delay = int(max_delay)

    def __len__(self):
        return int(self.cube.shape[0])

    def __repr__(self):
        K, nband, nsub, nbin = (int(s) for s in self.cube.shape)
        return "FoldedCandidates(%d candidates x %d bands x %d sub-integrations of %d samples x %d bins)" % (
            K, nband, nsub, self.L, nbin)

    def profile(self):
        """[K, nbin]: the cube summed over bands and sub-integrations."""
        return self.cube.sum((1, 2))

    def refine(self, ndrift=None, ndm=None, dm_step=None):
        """Refine the period and the DM of every candidate on its cube (host,
        float64, on a copy; the cube is all that crosses to the host).  With
        ``roll(v, r)[b] = v[(b + r) mod nbin]``, M / V the sums over the bands
        of ``mean`` / ``var`` and :func:`fold_chi2`:

        Period: ``A[s] = sum_g cube[g][s]``; for i in [-ndrift, ndrift]
        (default nbin // 4) a drift of i bins over the observation, taken at
        the centres of the sub-integrations, ``r_s(i) = (i (2 s + 1) + nsub) //
        (2 nsub)``; ``p_i = sum_s roll(A[s], r_s(i))`` and ``H_i`` the same sum
        over ``hits``; i* has the largest chi2(p_i, H_i), ties to the smaller
        |i|, then the smaller i.  ``period_opt = 1 / (1 / Ps - i* / (nbin nsub
        L))`` samples: a pulse that arrives later and later was folded at too
        short a period.

        DM: ``B[g] = sum_s roll(cube[g][s], r_s(i*))``; for m in [-ndm, ndm]
        (default nbin // 4) ``q_g(m) = floor(DM_K_VALUE m dm_step band_w[g] fs
        / Ps nbin + 1/2)`` bins, ``p_m = sum_g roll(B[g], q_g(m))``, judged by
        chi2(p_m, H_i*) under the same tie rule; ``dm_opt = dm + m* dm_step``.
        ``dm_step`` defaults to the DM offset that moves the band of largest
        ``band_w`` by one bin (0, and no search, when no band_w is positive).

        Returns a structured array, one row per candidate: ``period`` (s),
        ``dm``, ``chi2`` (at i = 0, m = 0), ``drift`` (i*), ``period_opt`` (s),
        ``dm_shift`` (m*), ``dm_opt``, ``chi2_opt``, ``peak_bin`` and
        ``profile`` (float64 [nbin], the refined profile p_m*).  The two
        searches are separable and move whole bins; period derivatives are not
        searched."""
        cube = np.array(_host(self.cube), dtype=np.float64)
        hits = np.array(_host(self.hits), dtype=np.float64)
        mean = np.array(_host(self.mean), dtype=np.float64)
        var = np.array(_host(self.var), dtype=np.float64)
        K, nband, nsub, nbin = cube.shape
        nd = nbin // 4 if ndrift is None else int(ndrift)
        nm = nbin // 4 if ndm is None else int(ndm)
        if nd < 0 or nm < 0:
            raise ValueError("refine: ndrift %d and ndm %d must not be negative" % (nd, nm))
        fs = float(self.samprate) * 1e6
        out = np.zeros(K, dtype=np.dtype([("period", np.float64), ("dm", np.float64), ("chi2", np.float64),
                                          ("drift", np.int64), ("period_opt", np.float64), ("dm_shift", np.int64),
                                          ("dm_opt", np.float64), ("chi2_opt", np.float64), ("peak_bin", np.int64),
                                          ("profile", np.float64, (nbin,))]))
        s_idx = np.arange(nsub)
        for k in range(K):
            Ps = float(self.period_samples[k])
            M, V = float(mean[k].sum()), float(var[k].sum())
            A = cube[k].sum(axis=0)                                       # [nsub][nbin]
            rs = lambda i: (i * (2 * s_idx + 1) + nsub) // (2 * nsub)
            prof = lambda rows, sh: sum(np.roll(rows[j], -int(sh[j])) for j in range(len(sh)))
            chis = [fold_chi2(prof(A, rs(i)), prof(hits[k], rs(i)), M, V) for i in range(-nd, nd + 1)]
            ibest = _fold_best(chis, nd)
            bands = lambda i: ([prof(cube[k, g], rs(i)) for g in range(nband)], prof(hits[k], rs(i)))
            B, H = bands(ibest)                                           # [nband][nbin], [nbin]
            step = dm_step
            if step is None:
                wmax = float(self.band_w.max())
                step = Ps / (DM_K_VALUE * wmax * fs * nbin) if wmax > 0 else 0.0
            step = float(step)
            qs = lambda m: [int(np.floor(DM_K_VALUE * m * step * self.band_w[g] * fs / Ps * nbin + 0.5))
                            for g in range(nband)]
            chim = [fold_chi2(prof(B, qs(m)), H, M, V) for m in range(-nm, nm + 1)]
            mbest = _fold_best(chim, nm)
            p = prof(B, qs(mbest))
            o = out[k]
            o["period"], o["dm"] = self.periods[k], self.dms[k]
            B0, H0 = bands(0)                                             # (the same operations as at i*, m*)
            o["chi2"] = fold_chi2(prof(B0, qs(0)), H0, M, V)
            o["drift"] = ibest
            o["period_opt"] = 1.0 / (1.0 / Ps - ibest / (float(nbin) * nsub * self.L)) / fs
            o["dm_shift"] = mbest
            o["dm_opt"] = self.dms[k] + mbest * step
            o["chi2_opt"] = chim[mbest + nm]
            o["peak_bin"] = int(np.argmax(p))
            o["profile"] = p
        return out


class Backend(object):
    def __init__(self, samprate=None, name=None):
        self._name = name
        self._samprate = make_quant(samprate, "MHz")

    def __repr__(self):
        return "Backend({:s})".format(self._name)

    @property
    def name(self):
        return self._name

    @property
    def samprate(self):
        return self._samprate

    def adc(self, signal):
        """backend.py:27-31 (unimplemented there too)."""

    @staticmethod
    def pfb_coefficients(Nchan, ntap):
        """Prototype filter of :meth:`channelize` (host, float64): ``ntap * L``
        coefficients, L = 2 Nchan.  ``ntap == 1``: all ones (a plain FFT
        filterbank); else ``sinc((i - (T L - 1)/2) / L) * hamming(T L)[i]``,
        scaled so that sum(h^2) = L -- unit-variance white noise then gives
        E|X_k|^2 = L for every ntap."""
        C, T = int(Nchan), int(ntap)
        if C < 1 or T < 1:
            raise ValueError("pfb_coefficients: Nchan %d, ntap %d" % (C, T))
        L = 2 * C
        if T == 1:
            return np.ones(L, dtype=np.float64)
        i = np.arange(T * L, dtype=np.float64)
        h = np.sinc((i - (T * L - 1) / 2.0) / L) * np.hamming(T * L)
        return h * np.sqrt(L / np.sum(h * h))

    @staticmethod
    def _channelize_plan(signal, Nchan, ntap, tscrunch):
        """Validate the arguments of :meth:`channelize` on the host (nothing
        touches the device): returns (C, T, tscrunch, Npol, N, S)."""
        if getattr(signal, "sigtype", None) != "BasebandSignal":
            raise ValueError("channelize takes a BasebandSignal, not %s"
                             % getattr(signal, "sigtype", type(signal).__name__))
        if signal._buf is None and signal._pending is None:
            raise ValueError("signal has no data: call Pulsar.make_pulses first")
        C, T, ts = int(Nchan), int(ntap), int(tscrunch)
        if C != Nchan or T != ntap or ts != tscrunch:
            raise ValueError("channelize: Nchan, ntap and tscrunch are integers")
        if C < 16 or C > 4096 or (C & (C - 1)):
            raise ValueError("channelize: Nchan %d is not a power of two in [16, 4096]" % C)
        if T < 1 or T > 8:
            raise ValueError("channelize: ntap %d outside [1, 8]" % T)
        if ts < 1:
            raise ValueError("channelize: tscrunch %d < 1" % ts)
        fs = signal._samprate_MHz()
        bw = float(to_value(signal.bw, 'MHz'))
        if fs != 2.0 * bw:
            raise ValueError("channelize: sample rate %r MHz is not 2 x the bandwidth %r MHz" % (fs, bw))
        npol = int(signal.Nchan)
        if npol not in (1, 2):
            raise ValueError("channelize: %d polarisation rows (1 or 2)" % npol)
        N = int(signal._ncols)
        M = N // (2 * C) - T + 1
        S = M // ts if M > 0 else 0
        if S < 1:
            raise ValueError("channelize: %d samples hold no output sample of %d spectra of %d points and %d taps"
                             % (N, ts, 2 * C, T))
        return C, T, ts, npol, N, S

    def channelize(self, signal, Nchan, ntap=1, tscrunch=1):
        """Channelise and detect a baseband signal on the device (extension:
        the reference has no counterpart -- its ``BasebandSignal.to_FilterBank``
        and ``Backend.adc`` are stubs).

        ``signal`` is a BasebandSignal with data, sampled at 2 x its bandwidth,
        of 1 or 2 polarisation rows.  With C = Nchan (a power of two in
        [16, 4096]), L = 2 C, T = ntap in [1, 8] and the prototype filter
        h = :meth:`pfb_coefficients` (C, T):

            y_m[j]    = sum_{t<T} h[t L + j] x[(m + t) L + j]
            X_m[k]    = sum_j y_m[j] exp(-2 pi i j k / L)
            out[k][s] = 1/(L tscrunch) sum_pol sum_{m in group s} |X_m[k]|^2

        for k < C (bin 0 kept, the Nyquist bin dropped): a polyphase (T > 1)
        or plain FFT (T = 1) filterbank, squared, summed over polarisations and
        ``tscrunch`` spectra.  Trailing samples and a ragged last group are
        dropped.  One fused kernel (``pss_channelize``): the voltages are read
        once and the powers written once, no host copy.

        Returns a new search-mode FilterBankSignal of C channels (channel k at
        ``fcent - bw/2 + k bw/C``) sampled at ``fs / (L tscrunch)``, with the
        attributes ``make_pulses`` gives a search-mode signal of that length,
        so ``fold_periods`` and search-mode ``PSRFITS.save`` accept it:
        ``sublen`` is the period of the pulsar whose ``make_pulses`` filled the
        voltages and ``nsub = round(tobs / period)``.  Voltages that came by
        another route carry no period; the result is then one subint
        spanning ``tobs`` (``nsub = 1``), and ``_Smax`` is None."""
        C, T, ts, npol, N, S = self._channelize_plan(signal, Nchan, ntap, tscrunch)
        from ..signal import FilterBankSignal
        data = signal.data                                    # flushes pending stages
        h = _engine.to_dev(self.pfb_coefficients(C, T).astype(np.float32))
        fs = signal._samprate_MHz()
        out_rate = fs / (2 * C * ts)
        fb = FilterBankSignal(to_value(signal.fcent, 'MHz'), to_value(signal.bw, 'MHz'), Nsubband=C, fold=False)
        fb._samprate = make_quant(out_rate, 'MHz')            # (set here: the constructor warns below Nyquist)
        # rows on the 16-B grid (a row stride of S rounded up to 4 samples): the
        # kernels that keep their accumulators in registers then store 16 B
        ld_out = (S + 3) // 4 * 4
        out = torch.empty((C, ld_out), dtype=torch.float32, device=data.device)[:, :S]
        rc = _lib.lib().pss_channelize(_engine.ptr(data), npol, N, max(int(data.stride(0)), N), _engine.ptr(h), C, T,
                                       ts, _engine.ptr(out), ld_out, _engine.stream_ptr())
        _lib.check(rc, "channelize")
        fb._buf = out
        fb._ncols = S
        fb._nsamp = S
        fb._pending = None
        tobs = S / (out_rate * 1e6)
        fb._tobs = make_quant(tobs, 's')
        # search mode as Pulsar._make_pow_pulses leaves it: one subint per
        # period of the pulsar the voltages were made with
        P = getattr(signal, "_period_s", None)
        if P:
            fb._sublen = make_quant(P, 's')
            fb._nsub = int(np.round(tobs / P))
        else:
            fb._sublen = fb._tobs
            fb._nsub = 1
        fb._set_draw_norm(df=1)
        fb._Smax = getattr(signal, "_Smax", None)
        fb._dm = signal._dm
        fb._delay = None
        fb._null_error = None
        fb._null_checks = []
        return fb

    @staticmethod
    def dedisperse_delays(signal, dms, ref_freq=None):
        """The integer delay table of :meth:`dedisperse` (host only, float64;
        nothing touches the device): int32 [nDM][C_local],

            x[j][c] = DM_K_VALUE * dms[j] * (f_c**-2 - f_ref**-2) [s] * samprate [Hz]
            d[j][c] = int(floor(x[j][c] + 0.5))

        with f_c the channel's entry in ``signal.dat_freq`` -- its lower edge,
        the frequency ``ISM.disperse`` delays it by -- so the DM that was
        injected undoes the sweep to within half a sample per channel.
        ``ref_freq`` (MHz) defaults to the largest ``dat_freq`` of the WHOLE
        band: the shards of a sharded signal (whose rows are
        ``local_dat_freq``) share one reference.  ValueError on an empty
        ``dms``, a negative or non-finite DM, a ``ref_freq`` below a channel
        frequency (negative delays) and a delay that does not fit in int32."""
        dm = np.atleast_1d(np.asarray(to_value(dms, 'pc/cm^3'), dtype=np.float64))
        if dm.ndim != 1 or dm.size < 1:
            raise ValueError("dedisperse: dms is empty or not one-dimensional")
        if not np.all(np.isfinite(dm)) or np.any(dm < 0):
            raise ValueError("dedisperse: a DM is negative or not finite")
        f_all = np.asarray(to_value(signal.dat_freq, 'MHz'), dtype=np.float64)
        f = np.asarray(to_value(getattr(signal, "local_dat_freq", signal.dat_freq), 'MHz'), dtype=np.float64)
        fref = float(np.max(f_all)) if ref_freq is None else float(to_value(ref_freq, 'MHz'))
        if not np.isfinite(fref) or fref <= 0 or np.any(f <= 0):
            raise ValueError("dedisperse: frequencies must be positive and finite")
        if np.any(f > fref):
            raise ValueError("dedisperse: ref_freq %r MHz is below a channel frequency (negative delays)" % fref)
        fs_hz = float(to_value(signal.samprate, 'MHz')) * 1e6
        x = DM_K_VALUE * dm[:, None] * (np.power(f, -2.0) - fref ** -2.0)[None, :] * fs_hz
        d = np.floor(x + 0.5)
        if not np.all(np.isfinite(d)) or d.max() > np.iinfo(np.int32).max:
            raise ValueError("dedisperse: a delay does not fit in int32")
        return d.astype(np.int32)

    @staticmethod
    def _dedisperse_plan(signal, dms, ref_freq=None):
        """Validate the arguments of :meth:`dedisperse` on the host (nothing
        touches the device): returns (dms, delays, ref_freq, max_delay, C, N)."""
        if getattr(signal, "sigtype", None) != "FilterBankSignal":
            raise ValueError("dedisperse takes a FilterBankSignal, not %s"
                             % getattr(signal, "sigtype", type(signal).__name__))
        if signal.fold:
            raise ValueError("dedisperse takes a search-mode signal (fold=False): a fold-mode buffer is tiled "
                             "sub-integrations, not a time series")
        if signal._buf is None and signal._pending is None:
            raise ValueError("signal has no data: call Pulsar.make_pulses first")
        dm = np.atleast_1d(np.asarray(to_value(dms, 'pc/cm^3'), dtype=np.float64))
        delays = Backend.dedisperse_delays(signal, dm, ref_freq)
        fref = (float(np.max(np.asarray(to_value(signal.dat_freq, 'MHz'), dtype=np.float64)))
                if ref_freq is None else float(to_value(ref_freq, 'MHz')))
        C, N = delays.shape[1], int(signal._ncols)
        max_delay = int(delays.max())
        if max_delay >= N:
            raise ValueError("dedisperse: the largest delay (%d samples) leaves no output sample of %d"
                             % (max_delay, N))
        return dm, delays, fref, max_delay, C, N

    def dedisperse(self, signal, dms, ref_freq=None):
        """Incoherent dedispersion over the trial DMs ``dms`` on the device
        (extension: the reference has no counterpart): the DM-time plane

            plane[j][t] = sum_c data[c][t + d[j][c]],   t < T = N - max(d)

        of a search-mode FilterBankSignal -- from ``make_pulses`` /
        ``ISM.disperse`` / ``observe`` or from :meth:`channelize` -- with
        d = :meth:`dedisperse_delays` (signal, dms, ref_freq).  One kernel
        (``pss_dedisperse``), the exact direct sum in a fixed order, no host
        copy of the data.  For a sharded signal the result is this rank's
        partial sum over its channels.  Returns a :class:`DedispersedPlane`."""
        dm, delays, fref, max_delay, C, N = self._dedisperse_plan(signal, dms, ref_freq)
        data = signal.data                                    # flushes pending stages
        if data.shape[0] != C:
            raise ValueError("dedisperse: %d data rows for %d channel frequencies" % (data.shape[0], C))
        tab = _engine.to_dev(delays)
        T = N - max_delay
        # rows on the 16-B grid, as channelize's: what reads the plane next can load 16 B
        ld_out = (T + 3) // 4 * 4
        out = torch.empty((delays.shape[0], ld_out), dtype=torch.float32, device=data.device)[:, :T]
        rc = _lib.lib().pss_dedisperse(_engine.ptr(data), C, N, max(int(data.stride(0)), N), _engine.ptr(tab),
                                       delays.shape[0], max_delay, _engine.ptr(out), ld_out, _engine.stream_ptr())
        _lib.check(rc, "dedisperse")
        return DedispersedPlane(out, dm, delays, signal._samprate_MHz(), fref, max_delay)

    @staticmethod
    def _search_plan(plane, nwidths=8, cell=32, threshold=6.0, dm_tol=1, time_tol=0, max_cells=1 << 20,
                     mean=None, std=None, stat_block=1024):
        """Validate the arguments of :meth:`boxcar_snr` and
        :meth:`single_pulse_search` on the host (nothing touches the device):
        returns (nDM, T, nwidths, cell, threshold, dm_tol, time_tol, max_cells,
        mean, std, stat_block), ``mean`` / ``std`` float64 [nDM] or None."""
        if not isinstance(plane, DedispersedPlane):
            raise ValueError("single-pulse search takes a DedispersedPlane, not %s" % type(plane).__name__)
        ndm, T = int(plane.data.shape[0]), int(plane.data.shape[1])
        if ndm < 1 or T < 1:
            raise ValueError("single-pulse search: the plane is empty (%d trials x %d samples)" % (ndm, T))
        try:
            nw, ce, sb, mc = int(nwidths), int(cell), int(stat_block), int(max_cells)
            ok = nw == nwidths and ce == cell and sb == stat_block and mc == max_cells
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError("single-pulse search: nwidths, cell, stat_block and max_cells are integers")
        if nw < 1 or nw > 13:
            raise ValueError("single-pulse search: nwidths %d outside [1, 13]" % nw)
        if ce < 16 or ce > 2048 or (ce & (ce - 1)):
            raise ValueError("single-pulse search: cell %d is not a power of two in [16, 2048]" % ce)
        if sb < 2:
            raise ValueError("single-pulse search: stat_block %d < 2" % sb)
        if mc < 0:
            raise ValueError("single-pulse search: max_cells %d < 0" % mc)
        th = float(threshold)
        if not np.isfinite(th) or th <= 0:
            raise ValueError("single-pulse search: threshold %r is not finite and positive" % (threshold,))
        if not (dm_tol >= 0) or not (time_tol >= 0):
            raise ValueError("single-pulse search: dm_tol %r and time_tol %r must not be negative"
                             % (dm_tol, time_tol))
        if (mean is None) != (std is None):
            raise ValueError("single-pulse search: give both mean and std, or neither")
        if mean is not None:
            stats = []
            for name, v in (("mean", mean), ("std", std)):
                a = np.asarray(v, dtype=np.float64)
                if a.ndim == 0:
                    a = np.full(ndm, float(a))
                if a.ndim != 1 or a.size != ndm:
                    raise ValueError("single-pulse search: %s has %s entries for %d trials"
                                     % (name, "x".join(str(s) for s in a.shape), ndm))
                if not np.all(np.isfinite(a)):
                    raise ValueError("single-pulse search: %s has an entry that is not finite" % name)
                stats.append(a)
            mean, std = stats
            if np.any(std <= 0):
                raise ValueError("single-pulse search: std has an entry <= 0")
        return ndm, T, nw, ce, th, dm_tol, time_tol, mc, mean, std, sb

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
        data = plane.data
        if data.dtype != torch.float32 or data.stride(1) != 1:
            data = data.to(torch.float32).contiguous()
        ld = max(int(data.stride(0)), T)
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
        # rows of whole 64-B segments
        out_ld = (nq + 15) // 16 * 16
        snr = torch.empty((ndm, out_ld), dtype=torch.float32, device=data.device)[:, :nq]
        code = torch.empty((ndm, out_ld), dtype=torch.int32, device=data.device)[:, :nq]
        rc = _lib.lib().pss_boxcar_search(_engine.ptr(data), ndm, T, ld, _engine.ptr(mean32), _engine.ptr(rstd32),
                                          nw, ce, _engine.ptr(snr), _engine.ptr(code), out_ld,
                                          _engine.stream_ptr())
        _lib.check(rc, "boxcar_search")
        q0 = torch.arange(nq, dtype=torch.int64, device=data.device) * ce
        time = q0[None, :] + (code & 0xFFFF).to(torch.int64)
        return BoxcarPlane(snr, time, code >> 16, code, mean_d, std_d, ce, plane)

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
        idx = torch.nonzero(cells.snr >= th)
        n = int(idx.shape[0])
        if n > mc:
            raise ValueError("single_pulse_search: %d cells at or above threshold %g exceed max_cells %d -- raise "
                             "the threshold" % (n, th, mc))
        j, q = idx[:, 0], idx[:, 1]
        packed = torch.stack((j, cells.time[j, q], cells.width_log2[j, q].to(torch.int64))).cpu().numpy()
        s = cells.snr[j, q].cpu().numpy()
        arr = candidates_from_cells(s, packed[0], packed[1], np.left_shift(1, packed[2]), plane.dms,
                                    plane.samprate, dm_tol, time_tol)
        return PulseCandidates(arr, cells, th)

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
                       max_cells=1 << 20, mean=None, std=None, stat_block=1024, max_bytes=1 << 30, spectrum=None):
        """Validate the arguments of :meth:`dm_spectrum`, :meth:`harmonic_snr`
        and :meth:`periodicity_search` on the host (nothing touches the
        device): returns a dict with ndm, T, nl (levels, log2(nharm) + 1), cell,
        nfft, nbin, n_used (samples of a trial that enter the transform), df
        (Hz), kmin, threshold, dm_tol, freq_tol, max_cells, mean, std (float64
        [nDM] or None), stat_block and chunk (trials per spectrum chunk)."""
        what = "periodicity search"
        if not isinstance(plane, DedispersedPlane):
            raise ValueError("%s takes a DedispersedPlane, not %s" % (what, type(plane).__name__))
        ndm, T = int(plane.data.shape[0]), int(plane.data.shape[1])
        if ndm < 1 or T < 2:
            raise ValueError("%s: the plane is too small (%d trials x %d samples)" % (what, ndm, T))
        try:
            nh, ce, sb, mc, mb = int(nharm), int(cell), int(stat_block), int(max_cells), int(max_bytes)
            ok = nh == nharm and ce == cell and sb == stat_block and mc == max_cells and mb == max_bytes
            nf = None if nfft is None else int(nfft)
            ok = ok and (nf is None or nf == nfft)
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError("%s: nharm, cell, nfft, stat_block, max_cells and max_bytes are integers" % what)
        if nh not in (1, 2, 4, 8, 16):
            raise ValueError("%s: nharm %d is not one of 1, 2, 4, 8, 16" % (what, nh))
        if ce < 16 or ce > 2048 or (ce & (ce - 1)):
            raise ValueError("%s: cell %d is not a power of two in [16, 2048]" % (what, ce))
        if sb < 2:
            raise ValueError("%s: stat_block %d < 2" % (what, sb))
        if mc < 0:
            raise ValueError("%s: max_cells %d < 0" % (what, mc))
        if spectrum is not None:
            shp = tuple(int(s) for s in spectrum.shape)
            if len(shp) != 2 or shp[0] != ndm or shp[1] < 2:
                raise ValueError("%s: spectrum has the shape %s for %d trials" % (what, "x".join(map(str, shp)), ndm))
            if nf is None:
                nf = 2 * (shp[1] - 1)
            elif shp[1] != nf // 2 + 1:
                raise ValueError("%s: spectrum has %d bins, nfft %d gives %d" % (what, shp[1], nf, nf // 2 + 1))
        if nf is None:
            nf = Backend.fft_length(T)
        if nf < 2 or nf % 2:
            raise ValueError("%s: nfft %d is not an even length >= 2" % (what, nf))
        nbin = nf // 2
        if nbin > 1 << 27:
            raise ValueError("%s: nfft %d gives more than 2^27 bins" % (what, nf))
        per_trial = (nbin + 1) * 8
        if mb < per_trial:
            raise ValueError("%s: max_bytes %d is below one trial's spectrum (%d bytes)" % (what, mb, per_trial))
        samprate = float(plane.samprate)
        df = samprate * 1e6 / nf
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
        th = float(threshold)
        if not np.isfinite(th) or th <= 0:
            raise ValueError("%s: threshold %r is not finite and positive" % (what, threshold))
        if not (dm_tol >= 0) or not (freq_tol >= 0):
            raise ValueError("%s: dm_tol %r and freq_tol %r must not be negative" % (what, dm_tol, freq_tol))
        if (mean is None) != (std is None):
            raise ValueError("%s: give both mean and std, or neither" % what)
        if mean is not None:
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
        return dict(ndm=ndm, T=T, nl=nh.bit_length(), cell=ce, nfft=nf, nbin=nbin, n_used=min(T, nf), df=df,
                    kmin=kmin, threshold=th, dm_tol=dm_tol, freq_tol=freq_tol, max_cells=mc, mean=mean, std=std,
                    stat_block=sb, chunk=max(1, min(ndm, mb // per_trial)))

    @staticmethod
    def _plane_rows(plane):
        data = plane.data
        if data.dtype != torch.float32 or data.stride(1) != 1:
            data = data.to(torch.float32).contiguous()
        return data, max(int(data.stride(0)), int(data.shape[1]))

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
        data, ld = self._plane_rows(plane)
        if mean is None:
            mean_d, _ = self._trial_stats(data, ld, p["stat_block"])
        elif isinstance(mean, torch.Tensor):
            mean_d = mean.to(device=data.device, dtype=torch.float64)
        else:
            m = np.asarray(mean, dtype=np.float64)
            m = np.full(p["ndm"], float(m)) if m.ndim == 0 else m
            if m.ndim != 1 or m.size != p["ndm"] or not np.all(np.isfinite(m)):
                raise ValueError("dm_spectrum: mean must hold %d finite entries" % p["ndm"])
            mean_d = _engine.to_dev(m)
            _engine.stream_ptr()                               # the stream waits for the upload
        if tuple(mean_d.shape) != (p["ndm"],):
            raise ValueError("dm_spectrum: mean has the shape %s for %d trials" % (tuple(mean_d.shape), p["ndm"]))
        lo, hi = (0, p["ndm"]) if trials is None else (int(trials[0]), int(trials[1]))
        if not (0 <= lo < hi <= p["ndm"]):
            raise ValueError("dm_spectrum: trials (%d, %d) outside [0, %d]" % (lo, hi, p["ndm"]))
        return self._spectrum_rows(data, mean_d.to(torch.float32), lo, hi, p["n_used"], p["nfft"])

    @staticmethod
    def _spectrum_rows(data, mean32, lo, hi, n_used, nfft):
        return torch.fft.rfft(data[lo:hi, :n_used] - mean32[lo:hi, None], n=nfft)

    def harmonic_snr(self, plane, nharm=16, cell=32, nfft=None, fmin=None, mean=None, std=None, stat_block=1024,
                     max_bytes=1 << 30, spectrum=None):
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
        the transform.  No host synchronisation."""
        p = self._harmonic_plan(plane, nharm=nharm, cell=cell, nfft=nfft, fmin=fmin, mean=mean, std=std,
                                stat_block=stat_block, max_bytes=max_bytes, spectrum=spectrum)
        ndm, ce, nbin = p["ndm"], p["cell"], p["nbin"]
        data, ld = self._plane_rows(plane)
        if p["mean"] is not None:
            mean_d, std_d = _engine.to_dev(p["mean"]), _engine.to_dev(p["std"])
            with np.errstate(all="ignore"):
                scale32 = _engine.to_dev((1.0 / (p["std"] * p["std"] * p["n_used"])).astype(np.float32))
            _engine.stream_ptr()                               # the stream waits for the uploads
        else:
            mean_d, var = self._trial_stats(data, ld, p["stat_block"])
            good = torch.isfinite(var) & (var > 0)
            std_d = torch.where(good, torch.sqrt(var), torch.zeros_like(var))
            # (from the std that is reported, as with user-given statistics)
            scale32 = torch.where(good, 1.0 / (std_d * std_d * p["n_used"]), torch.zeros_like(var)).to(torch.float32)
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
        # 8 and 16 harmonics: the kernel's power pass (half a spectrum chunk of workspace); below, gathering
        # from the spectrum itself is as fast or faster -- the same bits either way
        work = torch.empty(step * nbin, dtype=torch.float32, device=data.device) if p["nl"] > 3 else None
        for lo in range(0, ndm, step):
            hi = min(ndm, lo + step)
            spec = spec_all if spectrum is not None else self._spectrum_rows(data, mean32, lo, hi, p["n_used"],
                                                                             p["nfft"])
            rc = L.pss_harmonic_search(_engine.ptr(spec), hi - lo, nbin, int(spec.shape[1]),
                                       _engine.ptr(scale32[lo:hi]), p["nl"], p["kmin"], ce, _engine.ptr(snr[lo:hi]),
                                       _engine.ptr(code[lo:hi]), out_ld, _engine.ptr(work), _engine.stream_ptr())
            _lib.check(rc, "harmonic_search")
            del spec
        snr, code = snr[:, :nq], code[:, :nq]
        q0 = torch.arange(nq, dtype=torch.int64, device=data.device) * ce
        k = q0[None, :] + (code & 0xFFFF).to(torch.int64)
        lev = code >> 16
        freq = k.to(torch.float64) / torch.bitwise_left_shift(torch.ones_like(k), lev.to(torch.int64)) * p["df"]
        return HarmonicPlane(snr, k, lev, code, freq, p["df"], p["nfft"], nbin, p["kmin"], ce, mean_d, std_d, plane)

    def periodicity_search(self, plane, threshold=10.0, nharm=16, cell=32, dm_tol=1, freq_tol=1.0,
                           max_cells=1 << 20, nfft=None, fmin=None, mean=None, std=None, stat_block=1024,
                           max_bytes=1 << 30, spectrum=None):
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
        the number of (trial, bin, level) searched.  Returns
        :class:`PeriodCandidates`."""
        p = self._harmonic_plan(plane, nharm, cell, nfft, fmin, threshold, dm_tol, freq_tol, max_cells, mean, std,
                                stat_block, max_bytes, spectrum)
        cells = self.harmonic_snr(plane, nharm=nharm, cell=cell, nfft=nfft, fmin=fmin, mean=mean, std=std,
                                  stat_block=stat_block, max_bytes=max_bytes, spectrum=spectrum)
        th, mc = p["threshold"], p["max_cells"]
        idx = torch.nonzero(cells.snr >= th)
        n = int(idx.shape[0])
        if n > mc:
            raise ValueError("periodicity_search: %d cells at or above threshold %g exceed max_cells %d -- raise "
                             "the threshold" % (n, th, mc))
        j, q = idx[:, 0], idx[:, 1]
        packed = torch.stack((j, cells.bin[j, q], cells.nharm_log2[j, q].to(torch.int64))).cpu().numpy()
        s = cells.snr[j, q].cpu().numpy()
        arr = period_candidates_from_cells(s, packed[0], packed[1], packed[2], plane.dms, cells.df, p["dm_tol"],
                                           p["freq_tol"])
        return PeriodCandidates(arr, cells, th)

    @staticmethod
    def _accel_alpha(accel, samprate):
        """alpha = -a / (2 c fs) per sample as an exact Fraction of the float64
        inputs (fs = samprate [MHz] * 1e6, the float64 product)."""
        from fractions import Fraction
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
        from fractions import Fraction
        T = int(T)
        if T < 1:
            raise ValueError("acceleration search: T %d < 1" % T)
        al = Backend._accel_alpha(accel, samprate)
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
        kap = [Backend.accel_shift_step(a, samprate, T) for a in acc]
        # (T = 1 alone reaches 2^63; u(t) = 0 there)
        return acc, np.array([min(k, (1 << 63) - 1) for k in kap], dtype=np.int64)

    def _trial_mean(self, data, ld, ndm, mean, stat_block, what):
        """The per-trial baseline as a device float64 [nDM]: measured (block
        medians), a device tensor, or host values."""
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
        if not isinstance(plane, DedispersedPlane):
            raise ValueError("%s takes a DedispersedPlane, not %s" % (what, type(plane).__name__))
        data, ld = self._plane_rows(plane)
        ndm, T = int(data.shape[0]), int(data.shape[1])
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
        _engine.stream_ptr()                                   # the stream waits for the uploads
        sub_d = mean_d.to(torch.float32)[lo:hi].repeat_interleave(na)
        out_ld = (n + 3) // 4 * 4
        out = torch.empty((nt, na, out_ld), dtype=torch.float32, device=data.device)
        self._accel_launch(_lib.lib(), data, ndm, T, ld, src_d, kap_d, sub_d, nt * na, n, out, out_ld)
        return out[:, :, :n]

    def accel_snr(self, plane, accels, nharm=16, cell=32, nfft=None, fmin=None, mean=None, std=None,
                  stat_block=1024, max_bytes=1 << 30):
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
        :meth:`harmonic_snr`.  No host synchronisation.  Returns an
        :class:`AccelPlane`."""
        p = self._harmonic_plan(plane, nharm=nharm, cell=cell, nfft=nfft, fmin=fmin, mean=mean, std=std,
                                stat_block=stat_block, max_bytes=max_bytes)
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
        data, ld = self._plane_rows(plane)
        dev = data.device
        if p["mean"] is not None:
            mean_d, std_d = _engine.to_dev(p["mean"]), _engine.to_dev(p["std"])
            with np.errstate(all="ignore"):
                scale32 = _engine.to_dev((1.0 / (p["std"] * p["std"] * nu)).astype(np.float32))
        else:
            mean_d, var = self._trial_stats(data, ld, p["stat_block"])
            good = torch.isfinite(var) & (var > 0)
            std_d = torch.where(good, torch.sqrt(var), torch.zeros_like(var))
            scale32 = torch.where(good, 1.0 / (std_d * std_d * nu), torch.zeros_like(var)).to(torch.float32)
        # chunks: whole trials with all their accelerations, or one trial and a block of accelerations
        nt_c, na_c = (min(ndm, rows // na), na) if rows >= na else (1, rows)
        chunks = [(lo, min(ndm, lo + nt_c), a0, min(na, a0 + na_c))
                  for lo in range(0, ndm, nt_c) for a0 in range(0, na, na_c)]
        # one table for the call, the chunks' rows one after the other (trial-major, acceleration fastest)
        src_d = _engine.to_dev(np.concatenate([np.repeat(np.arange(lo, hi, dtype=np.int32), a1 - a0)
                                               for lo, hi, a0, a1 in chunks]))
        kap_d = _engine.to_dev(np.concatenate([np.tile(kap[a0:a1], hi - lo) for lo, hi, a0, a1 in chunks]))
        _engine.stream_ptr()                                   # the stream waits for the uploads
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
        L = _lib.lib()
        r0 = 0
        for lo, hi, a0, a1 in chunks:
            nt, nb = hi - lo, a1 - a0
            n = nt * nb
            self._accel_launch(L, data, ndm, T, ld, src_d[r0:r0 + n], kap_d[r0:r0 + n],
                               mean32[lo:hi].repeat_interleave(nb), n, nu, y, y_ld)
            spec = torch.fft.rfft(y[:n, :nu], n=p["nfft"])
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
        q0 = torch.arange(nq, dtype=torch.int64, device=dev) * ce
        k = q0[None, :] + (code & 0xFFFF).to(torch.int64)
        lev = code >> 16
        freq = k.to(torch.float64) / torch.bitwise_left_shift(torch.ones_like(k), lev.to(torch.int64)) * p["df"]
        return AccelPlane(snr, k, lev, code, freq, p["df"], p["nfft"], nbin, p["kmin"], ce, mean_d, std_d, plane,
                          bacc, acc)

    def accel_search(self, plane, accels=None, amax=None, threshold=10.0, nharm=16, cell=32, dm_tol=1,
                     freq_tol=1.0, max_cells=1 << 20, nfft=None, fmin=None, mean=None, std=None, stat_block=1024,
                     max_bytes=1 << 30, tol=1.0):
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
        well.  Returns :class:`AccelCandidates`."""
        if (accels is None) == (amax is None):
            raise ValueError("accel_search: give either accels or amax")
        p = self._harmonic_plan(plane, nharm, cell, nfft, fmin, threshold, dm_tol, freq_tol, max_cells, mean, std,
                                stat_block, max_bytes)
        if accels is None:
            accels = self.accel_trials(p["T"], plane.samprate, amax, tol)
        cells = self.accel_snr(plane, accels, nharm=nharm, cell=cell, nfft=nfft, fmin=fmin, mean=mean, std=std,
                               stat_block=stat_block, max_bytes=max_bytes)
        th, mc = p["threshold"], p["max_cells"]
        idx = torch.nonzero(cells.snr >= th)
        n = int(idx.shape[0])
        if n > mc:
            raise ValueError("accel_search: %d cells at or above threshold %g exceed max_cells %d -- raise the "
                             "threshold" % (n, th, mc))
        j, q = idx[:, 0], idx[:, 1]
        packed = torch.stack((j, cells.bin[j, q], cells.nharm_log2[j, q].to(torch.int64),
                              cells.acc_index[j, q].to(torch.int64))).cpu().numpy()
        s = cells.snr[j, q].cpu().numpy()
        base = period_candidates_from_cells(s, packed[0], packed[1], packed[2], plane.dms, cells.df, p["dm_tol"],
                                            p["freq_tol"])
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
        return AccelCandidates(arr, cells, th)

    @staticmethod
    def _phase_step(period_samples):
        """floor(2^64 / Ps + 1/2) as a Python int, Ps a float64 taken as the
        exact rational it is (host, integers only)."""
        from fractions import Fraction
        ps = float(period_samples)
        if not np.isfinite(ps) or ps <= 0:
            raise ValueError("fold: the period %r is not finite and positive" % (period_samples,))
        q = Fraction(1 << 64) / Fraction(ps) + Fraction(1, 2)
        return q.numerator // q.denominator

    @staticmethod
    def fold_phase_step(period, samprate):
        """The phase step of one sample of :meth:`fold_candidates` and
        ``pss_fold_series`` (host only): phases are 64-bit fixed point, a turn
        is 2^64, and with Ps = ``period`` [s] * ``samprate`` [MHz] * 1e6 (the
        float64 product, taken as an exact rational)

            inc    = floor(2^64 / Ps + 1/2)
            phi(u) = (phi0 + u inc) mod 2^64
            bin(u) = ((phi(u) >> 32) nbin) >> 32

        for sample u of the series.  Returns ``inc`` as a Python int, computed
        with integers: no float rounding enters a bin index."""
        return Backend._phase_step(float(to_value(period, 's')) * (float(to_value(samprate, 'MHz')) * 1e6))

    @staticmethod
    def _fold_plan(signal, candidates=None, dms=None, periods=None, nbin=64, nsub=16, nband=8, ref_freq=None,
                   stat_block=1024, max_candidates=64, max_bytes=1 << 30):
        """Validate the arguments of :meth:`fold_candidates` on the host
        (nothing touches the device): returns a dict with K, dms, periods,
        period_samples, inc (Python ints), udms (the unique DMs, rising), ju
        (candidate -> unique DM), delays (int32 [nudm][C]), ref_freq,
        max_delay, C, Cb (channels per band), N, T, L, ld (row stride of the
        sub-band series), band_w, nbin, nsub, nband, stat_block and chunks
        ([(lo, hi)) ranges of unique DMs whose sub-band series stay within
        ``max_bytes``)."""
        what = "fold_candidates"
        if getattr(signal, "sigtype", None) != "FilterBankSignal":
            raise ValueError("%s takes a FilterBankSignal, not %s"
                             % (what, getattr(signal, "sigtype", type(signal).__name__)))
        if signal.fold:
            raise ValueError("%s takes a search-mode signal (fold=False): a fold-mode buffer is tiled "
                             "sub-integrations, not a time series" % what)
        if signal._buf is None and signal._pending is None:
            raise ValueError("signal has no data: call Pulsar.make_pulses first")
        try:
            nb, ns, ng, sb, mc, mb = (int(nbin), int(nsub), int(nband), int(stat_block), int(max_candidates),
                                      int(max_bytes))
            ok = (nb == nbin and ns == nsub and ng == nband and sb == stat_block and mc == max_candidates
                  and mb == max_bytes)
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError("%s: nbin, nsub, nband, stat_block, max_candidates and max_bytes are integers" % what)
        if (candidates is None) == (dms is None and periods is None):
            raise ValueError("%s: give either candidates or dms and periods" % what)
        if candidates is not None:
            if not isinstance(candidates, PeriodCandidates):
                raise ValueError("%s: candidates is a %s, not PeriodCandidates" % (what, type(candidates).__name__))
            if mc < 1:
                raise ValueError("%s: max_candidates %d < 1" % (what, mc))
            arr = candidates.array
            arr = arr[np.argsort(-arr["snr"].astype(np.float64), kind="stable")[:mc]]
            dm, per = np.array(arr["dm"], dtype=np.float64), np.array(arr["period"], dtype=np.float64)
        else:
            if dms is None or periods is None:
                raise ValueError("%s: give both dms and periods" % what)
            dm = np.atleast_1d(np.asarray(to_value(dms, 'pc/cm^3'), dtype=np.float64))
            per = np.atleast_1d(np.asarray(to_value(periods, 's'), dtype=np.float64))
            if dm.ndim != 1 or per.ndim != 1 or dm.size != per.size:
                raise ValueError("%s: %d dms for %d periods" % (what, dm.size, per.size))
        K = int(dm.size)
        if K < 1:
            raise ValueError("%s: no candidate to fold" % what)
        if not np.all(np.isfinite(per)) or np.any(per <= 0):
            raise ValueError("%s: a period is not finite and positive" % what)
        if nb < 2 or nb > 1024:
            raise ValueError("%s: nbin %d outside [2, 1024]" % (what, nb))
        if ns < 1:
            raise ValueError("%s: nsub %d < 1" % (what, ns))
        if sb < 2:
            raise ValueError("%s: stat_block %d < 2" % (what, sb))
        fs_hz = float(to_value(signal.samprate, 'MHz')) * 1e6
        ps = per * fs_hz
        if np.any(ps < nb):
            raise ValueError("%s: a period of %.6g samples is shorter than nbin %d bins -- lower nbin"
                             % (what, float(ps.min()), nb))
        udms, ju = np.unique(dm, return_inverse=True)
        delays = Backend.dedisperse_delays(signal, udms, ref_freq)
        f_all = np.asarray(to_value(signal.dat_freq, 'MHz'), dtype=np.float64)
        f = np.asarray(to_value(getattr(signal, "local_dat_freq", signal.dat_freq), 'MHz'), dtype=np.float64)
        fref = float(np.max(f_all)) if ref_freq is None else float(to_value(ref_freq, 'MHz'))
        C, N = int(delays.shape[1]), int(signal._ncols)
        if ng < 1 or C % ng:
            raise ValueError("%s: nband %d does not divide the %d channels" % (what, ng, C))
        max_delay = int(delays.max())
        if max_delay >= N:
            raise ValueError("%s: the largest delay (%d samples) leaves no output sample of %d"
                             % (what, max_delay, N))
        T = N - max_delay
        if ns > T:
            raise ValueError("%s: nsub %d exceeds the %d samples of a series" % (what, ns, T))
        ld = (T + 3) // 4 * 4
        per_dm = ng * ld * 4
        if per_dm > mb:
            raise ValueError("%s: the sub-band series of one DM (%d bytes) exceed max_bytes %d" % (what, per_dm, mb))
        # (at most 65535 series a statistics call)
        step = max(1, min(int(udms.size), mb // per_dm, 65535 // ng))
        Cb = C // ng
        band_w = (np.power(f, -2.0) - fref ** -2.0).reshape(ng, Cb).mean(axis=1)
        return dict(K=K, dms=dm, periods=per, period_samples=ps, inc=[Backend._phase_step(v) for v in ps],
                    udms=udms, ju=np.asarray(ju, dtype=np.int64).reshape(-1), delays=delays, ref_freq=fref,
                    max_delay=max_delay, C=C, Cb=Cb, N=N, T=T, L=T // ns, ld=ld, band_w=band_w, nbin=nb, nsub=ns,
                    nband=ng, stat_block=sb,
                    chunks=[(lo, min(int(udms.size), lo + step)) for lo in range(0, int(udms.size), step)])

    def fold_candidates(self, signal, candidates=None, dms=None, periods=None, nbin=64, nsub=16, nband=8,
                        ref_freq=None, stat_block=1024, max_candidates=64, max_bytes=1 << 30):
        """Fold periodicity candidates on the device (extension: the reference
        has no counterpart -- its fold needs a whole number of samples per
        period and knows no DM): the phase x time x band cube of each candidate,
        on which one checks that the pulse is there in every sub-integration and
        every sub-band, and refines the period and the DM
        (:meth:`FoldedCandidates.refine`).

        ``signal`` is a search-mode FilterBankSignal.  ``candidates`` is a
        :class:`PeriodCandidates` whose ``max_candidates`` strongest rows (by
        ``snr``) are folded at their ``dm`` and ``period``; or give ``dms``
        and ``periods`` (s), K entries each.  The C channels form ``nband``
        sub-bands of C / nband neighbours.  For every unique DM the existing
        kernel (``pss_dedisperse``) sums each band over its slice of the table
        :meth:`dedisperse_delays` (signal, unique dms, ref_freq) -- with the
        table's global maximum, so every band has T = N - max_delay samples and
        all stay aligned to one ``ref_freq`` -- into ``sub[band][dm][T]``, in
        chunks of DMs that keep it within ``max_bytes``.  One
        ``pss_fold_series`` call per chunk then folds row (k, g) from the
        series of band g at candidate k's DM with the phase of
        :meth:`fold_phase_step` (period_k, samprate), phi0 = 0, into ``nsub``
        sub-integrations of L = T // nsub samples and ``nbin`` bins (the last
        T - nsub L samples are left out).  A period must span at least
        ``nbin`` samples.  Per (candidate, band) the block-median mean and
        variance of the series are measured as in :meth:`boxcar_snr`
        (``stat_block``).  The bits depend on neither the chunking nor the
        order of the candidates.  Only the tables cross to the device and
        nothing to the host.  For a sharded signal the cube is this rank's
        partial one over its own channels (its C local channels form the
        bands); adding up the ranks' cubes is left to the caller.  Returns
        :class:`FoldedCandidates`."""
        p = self._fold_plan(signal, candidates, dms, periods, nbin, nsub, nband, ref_freq, stat_block,
                            max_candidates, max_bytes)
        data = signal.data                                    # flushes pending stages
        K, ng, ns, nb, Cb, N, T, ld = p["K"], p["nband"], p["nsub"], p["nbin"], p["Cb"], p["N"], p["T"], p["ld"]
        if data.shape[0] != p["C"]:
            raise ValueError("fold_candidates: %d data rows for %d channel frequencies" % (data.shape[0], p["C"]))
        if data.dtype != torch.float32 or data.stride(1) != 1:
            data = data.to(torch.float32).contiguous()
        ld_in = max(int(data.stride(0)), N)
        L = _lib.lib()
        dev = data.device
        cube = torch.empty((K, ng, ns, nb), dtype=torch.float32, device=dev)
        hits = torch.empty((K, ns, nb), dtype=torch.int32, device=dev)
        mean = torch.empty((K, ng), dtype=torch.float64, device=dev)
        var = torch.empty((K, ng), dtype=torch.float64, device=dev)
        inc = np.array(p["inc"], dtype=np.uint64)
        for lo, hi in p["chunks"]:
            nu = hi - lo
            sub = torch.empty((ng, nu, ld), dtype=torch.float32, device=dev)
            for g in range(ng):
                tab = _engine.to_dev(p["delays"][lo:hi, g * Cb:(g + 1) * Cb])
                rc = L.pss_dedisperse(_engine.ptr(data[g * Cb:(g + 1) * Cb]), Cb, N, ld_in, _engine.ptr(tab), nu,
                                      p["max_delay"], _engine.ptr(sub[g]), ld, _engine.stream_ptr())
                _lib.check(rc, "dedisperse")
            series = sub.view(ng * nu, ld)
            m, v = self._trial_stats(series[:, :T], ld, p["stat_block"])
            ks = np.flatnonzero((p["ju"] >= lo) & (p["ju"] < hi))
            # row (k, g) reads series g nu + ju(k) - lo
            src = (np.arange(ng, dtype=np.int64)[None, :] * nu + (p["ju"][ks] - lo)[:, None]).astype(np.int32)
            src_d = _engine.to_dev(src.reshape(-1))
            inc_d = _engine.u64_to_i64_tensor(np.repeat(inc[ks], ng))
            kidx = _engine.to_dev(ks.astype(np.int64))
            part = torch.empty((ks.size, ng, ns, nb), dtype=torch.float32, device=dev)
            phits = torch.empty((ks.size, ng, ns, nb), dtype=torch.int32, device=dev)
            rc = L.pss_fold_series(_engine.ptr(series), ng * nu, T, ld, _engine.ptr(src_d), _engine.ptr(inc_d), None,
                                   ks.size * ng, ns, p["L"], nb, _engine.ptr(part), _engine.ptr(phits),
                                   _engine.stream_ptr())
            _lib.check(rc, "fold_series")
            sidx = src_d.to(torch.int64).view(ks.size, ng)
            cube.index_copy_(0, kidx, part)
            hits.index_copy_(0, kidx, phits[:, 0])
            mean.index_copy_(0, kidx, m[sidx])
            var.index_copy_(0, kidx, v[sidx])
            del sub, series, part, phits
        return FoldedCandidates(cube, hits, mean, var, p["dms"], p["periods"], p["period_samples"], p["inc"],
                                p["band_w"], signal._samprate_MHz(), p["ref_freq"], p["L"], T, p["max_delay"])

    def fold(self, signal, pulsar):
        """backend.py:34-49: Npbins = int(P * 2 * signal.samprate);
        sum over the N_fold blocks of Npbins//2 samples that follow the first
        Npbins samples.  As in the reference the reshape only succeeds when
        Nt - Npbins == N_fold * (Npbins//2), else ValueError."""
        data = signal.data
        Nf, Nt = data.shape
        P = float(to_value(pulsar.period, 's'))
        Npbins = int((P * 2 * signal._samprate_MHz()) * 1e6)
        N_fold = Nt // Npbins
        width = min(Nt, Npbins * (N_fold + 1)) - Npbins
        if width != N_fold * (Npbins // 2):
            raise ValueError("cannot reshape array of size %d into shape (%d,%d,%d)"
                             % (Nf * max(width, 0), Nf, N_fold, Npbins // 2))
        out = torch.empty((Nf, Npbins // 2), dtype=torch.float32, device=data.device)
        rc = _lib.lib().pss_fold(_engine.ptr(data), _engine.ptr(out), Nf, data.stride(0), Npbins,
                                 N_fold, _engine.stream_ptr())
        _lib.check(rc, "fold")
        return out

    def fold_periods(self, signal, pulsar, nbin=None):
        """Corrected fold (extension; the reference's ``fold`` above is only
        valid for exactly four periods): the sum of the signal over its whole
        periods of ``nbin`` samples (default ``int(P * samprate)``, the
        samples per period make_pulses uses), on the device.  Trailing samples
        of an incomplete period are dropped.  Returns [Nchan, nbin] float32."""
        data = signal.data
        Nf, Nt = data.shape
        if nbin is None:
            P = float(to_value(pulsar.period, 's'))
            nbin = int(P * signal._samprate_MHz() * 1e6)
        nbin = int(nbin)
        nper = Nt // nbin if nbin > 0 else 0
        if nbin < 1 or nper < 1:
            raise ValueError("fold_periods: %d samples hold no whole period of %d bins" % (Nt, nbin))
        out = torch.empty((Nf, nbin), dtype=torch.float32, device=data.device)
        rc = _lib.lib().pss_fold_periods(_engine.ptr(data), _engine.ptr(out), Nf, data.stride(0), nbin, nper,
                                         _engine.stream_ptr())
        _lib.check(rc, "fold_periods")
        return out
