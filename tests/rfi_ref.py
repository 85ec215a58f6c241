"""NumPy models of the RFI stage (psrsigsim_amd/telescope/rfi.py, csrc/pss_rficlean.hip), independent of torch
and of the device.

``mask_rule``  the four rules of ``Backend.rfi_mask`` in float64, one scalar at a time
``clean``      ``pss_rfi_clean`` in float32, operation for operation in the kernel's documented summation order
               (``clean64``: the same in float64, the yardstick of the float tests)

Medians are lower medians: sorted index (n - 1) // 2, a NaN sorting last (as np.sort and torch.sort put it).
"""
import numpy as np

MAD_SIGMA = 1.4826
Q = 8                      # the kernel's channel ranges: [q P, min((q + 1) P, C)), P = ceil(C / Q)


def lower_median(a):
    a = np.sort(np.asarray(a, dtype=np.float64))
    return a[(a.size - 1) // 2]


def block_stats(x, block):
    """(m, s, nb): mean and sqrt(max(var, 0)) [nb][C] of the whole blocks of x [C][N], float64."""
    x = np.asarray(x, dtype=np.float64)
    C, N = x.shape
    nb = N // block
    xb = x[:, :nb * block].reshape(C, nb, block)
    m = xb.sum(axis=2).T / block
    v = (xb * xb).sum(axis=2).T / block - m * m
    return m, np.sqrt(np.maximum(v, 0.0)), nb


def mask_rule(x, block=1024, thresh=5.0, chan_thresh=5.0, chan_window=17, chanfrac=0.5, intfrac=0.5,
              zap_chans=(), zap_blocks=()):
    """The mask of ``Backend.rfi_mask`` for x [C][N].  Returns a dict: ``mask`` bool [nb][C]; ``flags`` the
    flags of rules 1-3; ``m`` the block means; ``base`` float32 [C] and ``rgood`` float32 [nb] as RfiMask
    holds them; ``margin`` the smallest |lhs - rhs| / rhs over every threshold comparison lhs > rhs made
    (rhs > 0), ``cell_sigma`` / ``chan_sigma`` the deviations of rules 1 / 2 in units of their sigma
    ([2][nb][C] and [2][C]: for the mean and for the standard deviation)."""
    m, s, nb = block_stats(x, block)
    C = m.shape[1]
    w = chan_window // 2
    flags = np.zeros((nb, C), dtype=bool)
    margin = np.inf
    cell_sigma = np.zeros((2, nb, C))
    chan_sigma = np.zeros((2, C))
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, a in enumerate((m, s)):
            med = np.empty(C)
            for c in range(C):                                          # rule 1
                med[c] = lower_median(a[:, c])
                dev = np.abs(a[:, c] - med[c])
                sigma = MAD_SIGMA * lower_median(dev)
                lim = thresh * sigma
                for b in range(nb):
                    if dev[b] > lim or not np.isfinite(a[b, c]):
                        flags[b, c] = True
                    if lim > 0:
                        margin = min(margin, abs(dev[b] - lim) / lim)
                    cell_sigma[i, b, c] = dev[b] / sigma
            e = np.empty(C)
            for c in range(C):                                          # rule 2
                e[c] = abs(med[c] - lower_median(med[max(c - w, 0):min(c + w, C - 1) + 1]))
            sigma_e = MAD_SIGMA * lower_median(e)
            lim = chan_thresh * sigma_e
            for c in range(C):
                if e[c] > lim:
                    flags[:, c] = True
                if lim > 0:
                    margin = min(margin, abs(e[c] - lim) / lim)
                chan_sigma[i, c] = e[c] / sigma_e
    for c in zap_chans:                                                 # rule 3
        flags[:, c] = True
    for b in zap_blocks:
        flags[b, :] = True
    mask = flags.copy()                                                 # rule 4, both from `flags`
    for c in range(C):
        if flags[:, c].sum() > chanfrac * nb:
            mask[:, c] = True
    for b in range(nb):
        if flags[b, :].sum() > intfrac * C:
            mask[b, :] = True
    base, rgood = mask_tables(mask, m)
    return dict(mask=mask, flags=flags, m=m, base=base, rgood=rgood, margin=margin, cell_sigma=cell_sigma,
                chan_sigma=chan_sigma)


def mask_tables(mask, m):
    """(base float32 [C], rgood float32 [nb]): the lower median of a channel's unflagged block means (of all of
    them where none is unflagged; 0 where not finite), and float32(1 / unflagged channels), 0 where none."""
    nb, C = mask.shape
    base = np.zeros(C, dtype=np.float32)
    for c in range(C):
        keep = m[~mask[:, c], c]
        med = lower_median(keep if keep.size else m[:, c])
        base[c] = np.float32(med) if np.isfinite(med) else np.float32(0)
    rgood = np.zeros(nb, dtype=np.float32)
    for b in range(nb):
        good = C - int(mask[b].sum())
        rgood[b] = np.float32(1.0 / good) if good else np.float32(0)
    return base, rgood


MASK_CASE_BLOCK = 256


def mask_case(seed=0):
    """(x float32 [64][32868], injected bool [128][64]): chisquare(4) / 4 noise with a tone +0.5 on channel 5,
    a gain x3 on channel 20 in blocks 10-13, +20 on every channel for 8 samples of block 70 and +4 on channel
    40 for 64 samples of block 100; blocks of 256 samples (the last 100 samples are a ragged tail)."""
    C, N, block = 64, 32868, MASK_CASE_BLOCK
    x = (np.random.default_rng(seed).chisquare(4, size=(C, N)) / 4).astype(np.float32)
    inj = np.zeros((N // block, C), dtype=bool)
    x[5] += np.float32(0.5)
    inj[:, 5] = True
    x[20, 10 * block:14 * block] *= np.float32(3)
    inj[10:14, 20] = True
    x[:, 70 * block + 100:70 * block + 108] += np.float32(20)
    inj[70, :] = True
    x[40, 100 * block + 64:100 * block + 128] += np.float32(4)
    inj[100, 40] = True
    return x, inj


def sample_blocks(N, block, nblk):
    """b(t) = min(t // block, nblk - 1) for t < N."""
    return np.minimum(np.arange(N, dtype=np.int64) // block, nblk - 1)


def _clean(x, mask, block, base, rgood, zero_dm, order, dt):
    assert order == ("split", Q), order
    x = np.asarray(x, dtype=dt)
    base = np.asarray(base, dtype=dt)
    mask = np.asarray(mask) != 0
    C, N = x.shape
    nblk = mask.shape[0]
    bt = sample_blocks(N, block, nblk)
    good = ~mask[bt, :].T                                               # [C][N]
    out = np.empty((C, N), dtype=dt)
    z = np.zeros(N, dtype=dt)
    with np.errstate(invalid="ignore", over="ignore"):
        if zero_dm:
            P = (C + Q - 1) // Q
            A = []
            for q in range(Q):
                acc = np.zeros(N, dtype=dt)
                for c in range(min(q * P, C), min((q + 1) * P, C)):     # increasing c, flagged cells skipped
                    d = (x[c] - base[c]).astype(dt)
                    acc = np.where(good[c], (acc + d).astype(dt), acc)
                A.append(acc)
            lo = ((A[0] + A[1]).astype(dt) + (A[2] + A[3]).astype(dt)).astype(dt)
            hi = ((A[4] + A[5]).astype(dt) + (A[6] + A[7]).astype(dt)).astype(dt)
            S = (lo + hi).astype(dt)
            z = (S * np.asarray(rgood, dtype=dt)[bt]).astype(dt)
        for c in range(C):
            v = (x[c] - z).astype(dt) if zero_dm else x[c]
            out[c] = np.where(good[c], v, base[c])
    return out, z


def clean(x, mask, block, base, rgood, zero_dm, order=("split", Q)):
    """(out [C][N], z [N]) float32: pss_rfi_clean operation for operation (include/pss_hip.h)."""
    return _clean(x, mask, block, base, rgood, zero_dm, order, np.float32)


def clean64(x, mask, block, base, rgood, zero_dm, order=("split", Q)):
    """The same in float64 (float32 inputs widened exactly)."""
    return _clean(x, mask, block, base, rgood, zero_dm, order, np.float64)
