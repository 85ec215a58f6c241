"""RFI: put interference into a search-mode filterbank (``inject_rfi``) and take it out on the device
(``Backend.rfi_stats`` / ``rfi_mask`` / ``rfi_clean``: block statistics, an rfifind-style mask, replacement
of the flagged cells and removal of the zero-DM series)."""
import copy

import numpy as np
import torch

from .. import _engine, _lib
from .dedisperse import _check_search_signal
from .plane import _integers

MAD_SIGMA = 1.4826          # sigma of a normal distribution per median absolute deviation


def _lower_median(a, dim=0):
    """Lower median along ``dim`` (sorted index (n - 1) // 2; a NaN sorts last)."""
    return torch.sort(a, dim=dim).values.select(dim, (a.shape[dim] - 1) // 2)


def _running_lower_median(y, w):
    """Lower median of y over [c - w, c + w] clipped to [0, C): the window sorted (NaN last), index (len - 1) // 2."""
    C = int(y.shape[0])
    pad = torch.full((w,), float("nan"), dtype=y.dtype, device=y.device)
    win = torch.sort(torch.cat((pad, y, pad)).unfold(0, 2 * w + 1, 1), dim=1).values       # the padding sorts last
    c = torch.arange(C, device=y.device)
    length = torch.clamp(c + w, max=C - 1) - torch.clamp(c - w, min=0) + 1
    return win.gather(1, ((length - 1) // 2)[:, None])[:, 0]


class RfiMask(object):
    """Result of :meth:`Backend.rfi_mask`: which (block, channel) cells of a search-mode signal are interference.

    ``mask``   torch bool [nb, C] on the device, True = flagged; block b covers the samples [b block,
               (b + 1) block), the last one also the ragged tail up to ``nsamp``
    ``block``  samples per block;  ``nsamp`` samples of the signal the mask was made for
    ``base``   float32 [C]: the value a flagged cell is replaced by and the channel's baseline in the zero-DM
               sum -- the lower median of the block means of the channel's unflagged blocks (of all its
               blocks where none is unflagged; 0 where that is not finite)
    ``rgood``  float32 [nb]: 1 / (unflagged channels of the block), 0 where there is none
    ``frac``, ``chan_frac`` [C], ``block_frac`` [nb]: the flagged fraction of the cells, of each channel's blocks
               and of each block's channels"""

    def __init__(self, mask, block, nsamp, base, rgood):
        self.mask = mask
        self.block = int(block)
        self.nsamp = int(nsamp)
        self.base = base
        self.rgood = rgood

    @property
    def frac(self):
        return float(self.mask.double().mean())

    @property
    def chan_frac(self):
        return self.mask.double().mean(dim=0)

    @property
    def block_frac(self):
        return self.mask.double().mean(dim=1)

    def zapped_chans(self):
        """The channels flagged in every block (host int64 array)."""
        return torch.nonzero(self.mask.all(dim=0))[:, 0].cpu().numpy()

    def __repr__(self):
        nb, C = self.mask.shape
        return "RfiMask(%d blocks of %d samples x %d channels, %.3g %% flagged, %d channels zapped)" % (
            nb, self.block, C, 100.0 * self.frac, int(self.mask.all(dim=0).sum()))


def _mask_rules(m, v, th, cth, w, cf, tf, zc, zb):
    """The four rules of :meth:`RfiStage.rfi_mask` on the block means and variances (float64 [nb, C], on any
    device): the mask, bool [nb, C]."""
    nb, C = m.shape
    s = torch.sqrt(torch.clamp(v, min=0.0))
    flag = torch.zeros((nb, C), dtype=torch.bool, device=m.device)
    for a in (m, s):
        med = _lower_median(a)
        dev = torch.abs(a - med[None, :])
        sigma = MAD_SIGMA * _lower_median(dev)
        flag |= (dev > th * sigma[None, :]) | ~torch.isfinite(a)
        e = torch.abs(med - _running_lower_median(med, w))
        sigma_e = MAD_SIGMA * _lower_median(e)
        flag |= (e > cth * sigma_e)[None, :]
    if len(zc):
        flag[:, torch.as_tensor(zc, dtype=torch.int64, device=flag.device)] = True
    if len(zb):
        flag[torch.as_tensor(zb, dtype=torch.int64, device=flag.device), :] = True
    chan = flag.sum(dim=0).to(torch.float64) > cf * nb
    blk = flag.sum(dim=1).to(torch.float64) > tf * C
    return flag | chan[None, :] | blk[:, None]


def _mask_tables(mask, mean):
    """(base float32 [C], rgood float32 [nb]) of a mask [nb, C] and the block means (float64, device)."""
    nb, C = mask.shape
    kept = (~mask).sum(dim=0)                                                    # unflagged blocks per channel
    # an unflagged statistic is finite (rule 1), so +inf marks the flagged ones and sorts behind them
    srt = torch.sort(torch.where(mask, torch.full_like(mean, float("inf")), mean), dim=0).values
    med = srt.gather(0, (torch.clamp(kept, min=1) - 1)[None, :] // 2)[0]
    med = torch.where(kept > 0, med, _lower_median(mean))
    base = torch.where(torch.isfinite(med), med, torch.zeros_like(med)).to(torch.float32)
    good = (C - mask.sum(dim=1)).to(torch.float64)
    rgood = torch.where(good > 0, 1.0 / torch.clamp(good, min=1.0), torch.zeros_like(good)).to(torch.float32)
    return base, rgood


class RfiStage(object):
    @staticmethod
    def _rfi_stats_plan(signal, block, what="rfi_stats"):
        """Validate on the host (nothing touches the device): returns (block, nb, C, N)."""
        _check_search_signal(what, signal)
        block, = _integers(what, "block", block)
        N = int(signal._ncols)
        C = int(signal._c1 - signal._c0)
        if block < 16:
            raise ValueError("%s: block %d < 16" % (what, block))
        nb = N // block
        if nb < 4:
            raise ValueError("%s: %d samples hold %d whole blocks of %d (at least 4)" % (what, N, nb, block))
        return block, nb, C, N

    @staticmethod
    def _rfi_mask_plan(signal, block, thresh, chan_thresh, chan_window, chanfrac, intfrac, zap_chans, zap_blocks):
        """Validate the arguments of :meth:`rfi_mask` on the host: returns (block, nb, C, N, thresh, chan_thresh,
        w, chanfrac, intfrac, zap_chans int64 [..], zap_blocks int64 [..])."""
        what = "rfi_mask"
        block, nb, C, N = RfiStage._rfi_stats_plan(signal, block, what)
        th, cth = float(thresh), float(chan_thresh)
        if not (np.isfinite(th) and th > 0) or not (np.isfinite(cth) and cth > 0):
            raise ValueError("%s: thresh %r and chan_thresh %r must be finite and positive"
                             % (what, thresh, chan_thresh))
        cw, = _integers(what, "chan_window", chan_window)
        if cw < 1 or cw % 2 == 0:
            raise ValueError("%s: chan_window %d is not an odd number >= 1" % (what, cw))
        cf, tf = float(chanfrac), float(intfrac)
        if not (0 <= cf <= 1) or not (0 <= tf <= 1):
            raise ValueError("%s: chanfrac %r and intfrac %r lie in [0, 1]" % (what, chanfrac, intfrac))
        zaps = []
        for name, z, lim in (("zap_chans", zap_chans, C), ("zap_blocks", zap_blocks, nb)):
            a = np.atleast_1d(np.asarray(z))
            if a.size and (a.ndim != 1 or a.dtype.kind not in "iu"):
                raise ValueError("%s: %s holds integer indices" % (what, name))
            a = a.astype(np.int64).reshape(-1)
            if a.size and (a.min() < 0 or a.max() >= lim):
                raise ValueError("%s: %s has an index outside [0, %d)" % (what, name, lim))
            zaps.append(a)
        return block, nb, C, N, th, cth, cw // 2, cf, tf, zaps[0], zaps[1]

    @staticmethod
    def _rfi_clean_plan(signal, mask, zero_dm):
        """Validate the arguments of :meth:`rfi_clean` on the host: returns (C, N)."""
        what = "rfi_clean"
        _check_search_signal(what, signal)
        if not isinstance(mask, RfiMask):
            raise ValueError("%s takes an RfiMask, not %s" % (what, type(mask).__name__))
        N = int(signal._ncols)
        C = int(signal._c1 - signal._c0)
        nb, Cm = int(mask.mask.shape[0]), int(mask.mask.shape[1])
        if Cm != C:
            raise ValueError("%s: the mask has %d channels, the signal %d" % (what, Cm, C))
        if mask.nsamp != N:
            raise ValueError("%s: the mask was made for nsamp %d, the signal has %d" % (what, mask.nsamp, N))
        if mask.block < 1 or nb < 1 or nb != N // mask.block:
            raise ValueError("%s: %d blocks of block %d do not fit %d samples" % (what, nb, mask.block, N))
        if zero_dm and C != int(signal.Nchan):
            raise ValueError("%s: zero_dm needs the whole band; this shard holds channels [%d, %d) of %d "
                             "(mask replacement alone, zero_dm=False, works on a shard)"
                             % (what, signal._c0, signal._c1, int(signal.Nchan)))
        return C, N

    def rfi_stats(self, signal, block=1024):
        """Mean and variance of every (block, channel) cell of a search-mode signal on the device
        (``pss_chan_stats``, float64 sums in a fixed order): ``(mean, var)`` float64 [nb, C], nb = N // block
        whole blocks (trailing samples do not enter), var = sumsq / block - mean^2.  Needs nb >= 4, block >= 16."""
        block, nb, C, N = self._rfi_stats_plan(signal, block)
        data = signal.data
        if data.shape[0] != C:
            raise ValueError("rfi_stats: %d data rows for %d channels" % (data.shape[0], C))
        s1 = torch.empty((nb, C), dtype=torch.float64, device=data.device)
        s2 = torch.empty_like(s1)
        mn = torch.empty((nb, C), dtype=torch.float32, device=data.device)
        mx = torch.empty_like(mn)
        _lib.check(_lib.lib().pss_chan_stats(_engine.ptr(data), C, max(int(data.stride(0)), N), block, nb,
                                             _engine.ptr(mn), _engine.ptr(mx), _engine.ptr(s1), _engine.ptr(s2),
                                             _engine.stream_ptr()), "chan_stats")
        m = s1 / block
        return m, s2 / block - m * m

    def rfi_mask(self, signal, block=1024, thresh=5.0, chan_thresh=5.0, chan_window=17, chanfrac=0.5, intfrac=0.5,
                 zap_chans=(), zap_blocks=()):
        """An rfifind-style mask of a search-mode signal, computed on the device in float64 from the block
        statistics of :meth:`rfi_stats` (``m`` = mean, ``s`` = sqrt(max(var, 0)), both [nb, C]); medians are
        lower medians (sorted index (n - 1) // 2):

        1. cells, per channel over its blocks, for a in (m, s): med = median_b a, sigma = 1.4826 median_b
           |a - med|; flagged where |a - med| > thresh sigma (sigma = 0: every cell that differs) and where
           the statistic is not finite;
        2. channels, for y in (med_m, med_s): baseline[c] = median of y over the channels [c - w, c + w]
           clipped to the band, w = chan_window // 2; e = |y - baseline|, sigma_e = 1.4826 median_c e; the
           whole channel is flagged where e > chan_thresh sigma_e (a persistent carrier, which rule 1
           cannot see);
        3. ``zap_chans`` and ``zap_blocks`` (indices) are flagged whole;
        4. from the flags of 1-3: a channel flagged in more than ``chanfrac`` of its blocks is flagged whole,
           a block flagged in more than ``intfrac`` of its channels is flagged whole (both from the same
           flags: not cascaded).

        Returns an :class:`RfiMask`; nothing but scalars for its ``repr`` crosses to the host."""
        block, nb, C, N, th, cth, w, cf, tf, zc, zb = self._rfi_mask_plan(
            signal, block, thresh, chan_thresh, chan_window, chanfrac, intfrac, zap_chans, zap_blocks)
        m, v = self.rfi_stats(signal, block)
        mask = _mask_rules(m, v, th, cth, w, cf, tf, zc, zb)
        base, rgood = _mask_tables(mask, m)
        return RfiMask(mask, block, N, base, rgood)

    def rfi_clean(self, signal, mask, zero_dm=True, inplace=False, return_series=False):
        """Excise the interference an :class:`RfiMask` marks, on the device (one kernel, ``pss_rfi_clean``;
        IEEE float32, a fixed summation order, no atomics): every flagged (block, channel) cell becomes the
        channel's ``mask.base`` and, with ``zero_dm``, the zero-DM series

            z[t] = rgood[b(t)] * sum_{c unflagged} (data[c][t] - base[c])

        -- the band average of the unflagged channels about their baselines -- is subtracted from every
        unflagged sample: a broadband impulse at DM 0 goes before dedispersion smears it over every trial.
        The ragged tail behind the last whole block belongs to the last block.

        Returns a new search-mode FilterBankSignal with the metadata of ``signal`` (rows on the 16-B grid),
        or ``signal`` itself with ``inplace=True``; with ``return_series=True`` the pair (signal, z [N]
        float32 on the device; zeros without ``zero_dm``).  ValueError for a fold-mode or empty signal, a
        mask that does not fit it, and ``zero_dm`` on a shard that is not the whole band."""
        C, N = self._rfi_clean_plan(signal, mask, zero_dm)
        data = signal.data                                    # flushes pending stages
        if data.shape[0] != C:
            raise ValueError("rfi_clean: %d data rows for %d channels" % (data.shape[0], C))
        ld = max(int(data.stride(0)), N)
        if inplace:
            out, out_ld, res = data, ld, signal
        else:
            out_ld = (N + 3) // 4 * 4
            out = torch.empty((C, out_ld), dtype=torch.float32, device=data.device)[:, :N]
            res = copy.copy(signal)
            res._buf = out
            res._pending = None
            res._row0 = None
            res._null_error = None
            res._null_checks = []
        mbytes = mask.mask.to(device=data.device, dtype=torch.uint8).contiguous()
        base = mask.base.to(device=data.device, dtype=torch.float32).contiguous()
        rgood = mask.rgood.to(device=data.device, dtype=torch.float32).contiguous()
        z = None
        if return_series:
            z = (torch.empty if zero_dm else torch.zeros)((N,), dtype=torch.float32, device=data.device)
        rc = _lib.lib().pss_rfi_clean(_engine.ptr(data), C, N, ld, _engine.ptr(mbytes), mask.block,
                                      int(mbytes.shape[0]), _engine.ptr(base), _engine.ptr(rgood) if zero_dm else None,
                                      1 if zero_dm else 0, _engine.ptr(out), out_ld,
                                      _engine.ptr(z) if zero_dm else None, _engine.stream_ptr())
        _lib.check(rc, "rfi_clean")
        return (res, z) if return_series else res


def inject_rfi(signal, tones=(), bursts=(), impulses=()):
    """Put interference into a search-mode FilterBankSignal, in place on ``signal.data`` (deterministic, plain
    torch; the simulator's side of :meth:`Backend.rfi_clean`):

    ``tones``     (chan, add): a persistent carrier, ``add`` on every sample of the channel
    ``bursts``    (chan, t0, t1, gain): the samples [t0, t1) of the channel times ``gain``
    ``impulses``  (t0, width, add): ``add`` on the samples [t0, t0 + width) of every channel (zero DM)

    applied in that order.  Channels are rows of this process's data.  ValueError on an index outside the
    data (nothing is changed then).  Returns ``signal``."""
    _check_search_signal("inject_rfi", signal)
    N = int(signal._ncols)
    C = int(signal._c1 - signal._c0)
    plan = []
    for c, add in tones:
        c, = _integers("inject_rfi", "tone channels", c)
        if not 0 <= c < C:
            raise ValueError("inject_rfi: tone channel %d outside [0, %d)" % (c, C))
        plan.append(("add", slice(c, c + 1), slice(0, N), float(add)))
    for c, t0, t1, gain in bursts:
        c, t0, t1 = _integers("inject_rfi", "burst channels and times", c, t0, t1)
        if not 0 <= c < C:
            raise ValueError("inject_rfi: burst channel %d outside [0, %d)" % (c, C))
        if not 0 <= t0 < t1 <= N:
            raise ValueError("inject_rfi: burst samples [%d, %d) outside [0, %d)" % (t0, t1, N))
        plan.append(("mul", slice(c, c + 1), slice(t0, t1), float(gain)))
    for t0, width, add in impulses:
        t0, width = _integers("inject_rfi", "impulse times and widths", t0, width)
        if width < 1 or not 0 <= t0 <= N - width:
            raise ValueError("inject_rfi: impulse samples [%d, %d) outside [0, %d)" % (t0, t0 + width, N))
        plan.append(("add", slice(0, C), slice(t0, t0 + width), float(add)))
    data = signal.data
    for op, rows, cols, v in plan:
        if op == "add":
            data[rows, cols] += v
        else:
            data[rows, cols] *= v
    return signal
