"""Candidate folding: the phase x time x band cube of periodicity candidates, and its refinement."""
import numpy as np
import torch

from .._units import to_value
from ..utils.constants import DM_K_VALUE
from .. import _engine, _lib
from .plane import PlaneStage, _host, _integers
from .dedisperse import DedisperseStage, _check_search_signal, _ref_freq
from .periodicity import PeriodCandidates


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


class FoldStage(PlaneStage):
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
        return FoldStage._phase_step(float(to_value(period, 's')) * (float(to_value(samprate, 'MHz')) * 1e6))

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
        _check_search_signal(what, signal)
        nb, ns, ng, sb, mc, mb = _integers(what, "nbin, nsub, nband, stat_block, max_candidates and max_bytes", nbin,
                                           nsub, nband, stat_block, max_candidates, max_bytes)
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
        delays = DedisperseStage.dedisperse_delays(signal, udms, ref_freq)
        f = np.asarray(to_value(getattr(signal, "local_dat_freq", signal.dat_freq), 'MHz'), dtype=np.float64)
        fref = _ref_freq(signal, ref_freq)
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
        return dict(K=K, dms=dm, periods=per, period_samples=ps, inc=[FoldStage._phase_step(v) for v in ps],
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
        data, ld_in = self._plane_rows(data)
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
