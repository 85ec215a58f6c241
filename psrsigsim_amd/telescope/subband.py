"""Sub-band dedispersion: the DM-time plane in two stages -- bands at nominal DMs, then trials from bands."""
import numpy as np
import torch

from .. import _engine, _lib
from .plane import DedispersedPlane, _integers
from .dedisperse import DedisperseStage, _check_search_signal, _ref_freq
from .._units import to_value


class SubbandPlan(object):
    """The tables of :meth:`Backend.subband_dedisperse` (host, int64 arithmetic; see :meth:`Backend.subband_plan`).

    ``nsub``, ``group``  bands of C / nsub neighbouring channels; trials per nominal DM
    ``nominal``          int64 [ngroups], the nominal trial n_g of each group
    ``ref_chan``         int64 [nsub], the reference channel r(s) of each band
    ``d1``               int32 [ngroups][C], stage 1: a channel against its band's reference at the nominal trial
    ``d2``               int32 [nDM][nsub], stage 2: the band's reference at the trial itself
    ``delays``           int32 [nDM][C], the effective table e = d1[g(j)] + d2[j][s(c)]
    ``smear``            max |e - D| over the table, samples (D = ``dedisperse_delays``)
    ``m1``, ``m2``       max d1, max d2;  ``T1`` = N - m1, ``T`` = N - m1 - m2 output samples
    ``adds_direct``      nDM * C, the direct sum's additions per output sample
    ``adds_subband``     ngroups * C + nDM * nsub, this scheme's"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "SubbandPlan(%d bands, groups of %d trials, smear %d, %.3f of the direct additions)" % (
            self.nsub, self.group, self.smear, self.adds_subband / self.adds_direct)


def _ref_channels(f, nsub):
    """r(s): the channel of largest frequency of each band, ties to the lowest index."""
    band = f.size // nsub
    return np.arange(nsub, dtype=np.int64) * band + np.argmax(f.reshape(nsub, band), axis=1)


def _tables(D, ref, nsub, group):
    """(nominal, d1, d2, e) of the int64 table D [nDM][C] for the reference channels ``ref``."""
    ndm, C = D.shape
    lo = np.arange(0, ndm, group, dtype=np.int64)
    nominal = (lo + np.minimum(lo + group, ndm) - 1) // 2
    d2 = D[:, ref]
    d1 = D[nominal] - np.repeat(D[nominal][:, ref], C // nsub, axis=1)
    e = np.repeat(d1, group, axis=0)[:ndm] + np.repeat(d2, C // nsub, axis=1)
    return nominal, d1, d2, e


class SubbandStage(object):
    @staticmethod
    def subband_plan(signal, dms, nsub=None, group=None, max_smear=2.0, ref_freq=None):
        """The plan of :meth:`subband_dedisperse` (host only; nothing touches
        the device).  With D = :meth:`dedisperse_delays` (signal, dms,
        ref_freq), int64 [nDM][C]: the C channels form ``nsub`` bands of
        band = C / nsub neighbours, s(c) = c // band, with the reference channel
        r(s) the band's channel of largest ``dat_freq`` (ties to the lowest
        index); the trials, in the order given, form groups of ``group``
        consecutive ones (the last may be short), g(j) = j // group, with the
        nominal trial n_g = (lo + hi) // 2 of the group's trials lo .. hi:

            d1[g][c] = D[n_g][c] - D[n_g][r(s(c))]      (>= 0)
            d2[j][s] = D[j][r(s)]
            e[j][c]  = d1[g(j)][c] + d2[j][s(c)]
            m1 = max d1, m2 = max d2, T1 = N - m1, T = N - m1 - m2

        e is the table the two stages sum over, exactly; it equals D at the
        nominal trials and the reference channels and elsewhere |e - D| <
        |delta| + 2, delta the same combination of the unrounded delays.

        ``nsub`` and ``group``, when given, are checked (nsub divides C; group
        >= 1) and used as they are.  For one left ``None`` the choice is among
        nsub in the powers of two that divide C with band >= 2 and group in
        {8, 16, 32, ..} <= max(8, nDM): the pair of fewest ``adds_subband``
        whose ``smear`` <= ``max_smear``, ties to the fewer bands, then to the
        smaller group; ValueError, naming the smallest smear reached, when
        there is none.  The other argument errors are :meth:`dedisperse`'s.
        Returns a :class:`SubbandPlan`."""
        what = "subband_dedisperse"
        _check_search_signal(what, signal)
        dm = np.atleast_1d(np.asarray(to_value(dms, 'pc/cm^3'), dtype=np.float64))
        D = DedisperseStage.dedisperse_delays(signal, dm, ref_freq).astype(np.int64)
        f = np.asarray(to_value(getattr(signal, "local_dat_freq", signal.dat_freq), 'MHz'), dtype=np.float64)
        ndm, C = D.shape
        N = int(signal._ncols)
        ms = float(max_smear)
        if not ms >= 0:
            raise ValueError("%s: max_smear %r is negative or not a number" % (what, max_smear))
        if nsub is not None:
            nsub, = _integers(what, "nsub and group", nsub)
            if nsub < 1 or C % nsub:
                raise ValueError("%s: nsub %d does not divide the %d channels" % (what, nsub, C))
        if group is not None:
            group, = _integers(what, "nsub and group", group)
            if group < 1:
                raise ValueError("%s: group %d < 1" % (what, group))
        subs = [nsub] if nsub is not None else [s for s in (1 << k for k in range(32)) if 2 * s <= C and C % s == 0]
        groups = [group] if group is not None else [8 << k for k in range(32) if (8 << k) <= max(8, ndm)]
        if not subs:
            raise ValueError("%s: %d channels form no band of at least 2" % (what, C))
        best, reached = None, None
        for s in subs:
            ref = _ref_channels(f, s)
            for g in groups:
                nominal, d1, d2, e = _tables(D, ref, s, g)
                smear = int(np.abs(e - D).max())
                reached = smear if reached is None else min(reached, smear)
                adds = d1.shape[0] * C + ndm * s
                if (nsub is None or group is None) and smear > ms:
                    continue
                if best is None or (adds, s, g) < best[0]:
                    best = ((adds, s, g), ref, nominal, d1, d2, e, smear)
        if best is None:
            raise ValueError("%s: no choice of nsub and group keeps the smear within max_smear %g samples "
                             "(the smallest reached is %d)" % (what, ms, reached))
        (adds, s, g), ref, nominal, d1, d2, e, smear = best
        m1, m2 = int(d1.max()), int(d2.max())
        if N - m1 - m2 < 1:
            raise ValueError("%s: the largest delay (%d samples) leaves no output sample of %d" % (what, m1 + m2, N))
        # (C-contiguous: a column gather such as D[:, ref] need not be, and the tables go to the device as they lie)
        d1, d2, e = (np.ascontiguousarray(a, dtype=np.int32) for a in (d1, d2, e))
        return SubbandPlan(nsub=s, group=g, nominal=nominal, ref_chan=ref, d1=d1, d2=d2, delays=e, smear=smear, m1=m1,
                           m2=m2, T1=N - m1,
                           T=N - m1 - m2, adds_direct=ndm * C, adds_subband=adds, dms=dm,
                           ref_freq=_ref_freq(signal, ref_freq))

    @staticmethod
    def _subband_chunks(plan, max_bytes):
        """[(g_lo, g_hi)): whole groups whose band series sub[groups][nsub][T1 rounded up to 4] float32 stay within
        ``max_bytes``; ValueError if one group does not fit."""
        what = "subband_dedisperse"
        mb, = _integers(what, "max_bytes", max_bytes)
        per_group = plan.nsub * ((plan.T1 + 3) // 4 * 4) * 4
        if per_group > mb:
            raise ValueError("%s: the band series of one group (%d bytes) exceed max_bytes %d" % (what, per_group, mb))
        ng = int(plan.d1.shape[0])
        step = min(ng, mb // per_group)
        return [(lo, min(ng, lo + step)) for lo in range(0, ng, step)]

    def subband_dedisperse(self, signal, dms, nsub=None, group=None, max_smear=2.0, ref_freq=None,
                           max_bytes=2 ** 31):
        """Two-stage sub-band dedispersion on the device (extension: the
        reference has no counterpart): the DM-time plane of :meth:`dedisperse`
        for about ``adds_subband / adds_direct`` of its additions, over a
        delay table that differs from the exact one by at most ``smear``
        samples.  With the tables of :meth:`subband_plan` (same arguments):

            sub[g][s][u] = sum_{c in band s} data[c][u + d1[g][c]],       u < T1
            plane[j][t]  = sum_s             sub[g(j)][s][t + d2[j][s]],  t < T

        so ``plane`` is exactly the direct sum of the data over the effective
        table e = ``plan.delays`` with max_delay = m1 + m2; only the order of
        the float32 additions differs from ``pss_dedisperse`` on that table (a
        band's channels in increasing c, then the bands in increasing s).  m1 +
        m2 may differ from max(D) by a few samples, so T = N - m1 - m2 is not
        always :meth:`dedisperse`'s T.

        The groups are taken in chunks of whole groups whose band series
        sub[groups][nsub][T1 rounded up to 4] stay within ``max_bytes``
        (ValueError if one group does not fit); each chunk is two launches of
        ``pss_dedisperse_banded``, and the plane's bits do not depend on the
        chunking.  No host copy of the data.  For a sharded signal the result
        is this rank's partial sum over its own channels (which form the
        bands).  Returns a :class:`DedispersedPlane` whose ``delays`` is e,
        whose ``max_delay`` is m1 + m2 and whose ``subband`` is the plan:
        every search stage takes it as it stands."""
        plan = self.subband_plan(signal, dms, nsub, group, max_smear, ref_freq)
        chunks = self._subband_chunks(plan, max_bytes)
        data = signal.data                                    # flushes pending stages
        ndm, C = plan.delays.shape
        N = plan.T1 + plan.m1
        if data.shape[0] != C:
            raise ValueError("subband_dedisperse: %d data rows for %d channel frequencies" % (data.shape[0], C))
        ld = max(int(data.stride(0)), N)
        T1, T, ns, grp = plan.T1, plan.T, plan.nsub, plan.group
        ld1, ld_out = (T1 + 3) // 4 * 4, (T + 3) // 4 * 4
        t1, t2 = _engine.to_dev(plan.d1), _engine.to_dev(plan.d2)
        sub = torch.empty((max(hi - lo for lo, hi in chunks), ns, ld1), dtype=torch.float32, device=data.device)
        out = torch.empty((ndm, ld_out), dtype=torch.float32, device=data.device)[:, :T]
        L = _lib.lib()
        for lo, hi in chunks:
            j0, j1 = lo * grp, min(ndm, hi * grp)
            # stage 1: one source, the chunk's nominal trials, bands of C / nsub channels
            rc = L.pss_dedisperse_banded(_engine.ptr(data), 1, C * ld, C, N, ld, _engine.ptr(t1[lo:hi]), hi - lo,
                                         hi - lo, plan.m1, C // ns, _engine.ptr(sub), ld1, _engine.stream_ptr())
            _lib.check(rc, "dedisperse_banded")
            # stage 2: a source per group, its trials summed over the nsub band series
            rc = L.pss_dedisperse_banded(_engine.ptr(sub), hi - lo, ns * ld1, ns, T1, ld1, _engine.ptr(t2[j0:j1]),
                                         j1 - j0, grp, plan.m2, ns, _engine.ptr(out[j0:j1]), ld_out,
                                         _engine.stream_ptr())
            _lib.check(rc, "dedisperse_banded")
        plane = DedispersedPlane(out, plan.dms, plan.delays, signal._samprate_MHz(), plan.ref_freq, plan.m1 + plan.m2)
        plane.subband = plan
        return plane
