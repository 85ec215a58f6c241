"""NumPy restatement of the single-pulse search (no GPU, no package code):

* ``boxcar_ref``     -- ``pss_boxcar_search`` (include/pss_hip.h) in float32, one
  rounded operation per line: the mean subtracted, the balanced summation tree
  ``S = S[:-h] + S[h:]`` level by level, the explicit ``c[j][k] = a_k * rstd[j]``,
  and per cell the lexicographic maximum of (z, -k, -t);
* ``block_median_stats`` -- the per-trial statistics of ``Backend.boxcar_snr``
  in float64;
* ``cluster_all_pairs`` / ``candidates_ref`` -- friends-of-friends by testing
  every pair, and the candidate of each cluster.
"""
import numpy as np

SQRT2_F32 = np.array([0x3FB504F3], dtype=np.uint32).view(np.float32)[0]


def coef(k):
    """a_k = 2^-ceil(k/2) * (k odd ? float32(sqrt 2) : 1), exact in float32."""
    s = SQRT2_F32 if k & 1 else np.float32(1.0)
    return np.float32(np.ldexp(np.float64(s), -((k + 1) // 2)))


def best_per_time(row, mean, rstd, nw):
    """(z, k) float32 / int32 [T]: per start time the largest z_k[t] over the
    widths that fit, the narrower on ties; -inf, 0 where nothing beat -inf."""
    T = row.size
    with np.errstate(all="ignore"):
        S = row.astype(np.float32) - np.float32(mean)
        bz = np.full(T, -np.inf, dtype=np.float32)
        bk = np.zeros(T, dtype=np.int32)
        for k in range(nw):
            h = 1 << k
            if h > T:
                break
            assert S.size == T - h + 1 and S.dtype == np.float32
            c = np.float32(coef(k) * np.float32(rstd))
            z = S * c
            assert z.dtype == np.float32
            upd = z > bz[:z.size]                      # (a NaN never compares greater)
            bz[:z.size][upd] = z[upd]
            bk[:z.size][upd] = k
            if 2 * h > T:
                break
            S = S[:-h] + S[h:]
    return bz, bk


def boxcar_ref(plane, mean, rstd, nw, cell):
    """snr float32 [ndm][nq], code int32 [ndm][nq] of pss_boxcar_search."""
    plane = np.asarray(plane, dtype=np.float32)
    ndm, T = plane.shape
    mean = np.broadcast_to(np.asarray(mean, dtype=np.float32), (ndm,))
    rstd = np.broadcast_to(np.asarray(rstd, dtype=np.float32), (ndm,))
    nq = -(-T // cell)
    snr = np.full((ndm, nq), -np.inf, dtype=np.float32)
    code = np.zeros((ndm, nq), dtype=np.int32)
    toff = np.arange(nq * cell, dtype=np.int64).reshape(nq, cell) % cell
    for j in range(ndm):
        bz, bk = best_per_time(plane[j], mean[j], rstd[j], nw)
        z = np.full(nq * cell, -np.inf, dtype=np.float32)
        z[:T] = bz
        kk = np.zeros(nq * cell, dtype=np.int64)
        kk[:T] = bk
        z, kk = z.reshape(nq, cell), kk.reshape(nq, cell)
        top = z.max(axis=1)                              # (no NaN is ever stored)
        key = np.where(z == top[:, None], (kk << 16) | toff, np.int64(1) << 40)
        pos = key.argmin(axis=1)                         # narrower width, then earlier time
        snr[j] = z[np.arange(nq), pos]                   # the winner's own bits (-0.0 stays -0.0)
        code[j] = np.where(top == -np.inf, 0, key[np.arange(nq), pos]).astype(np.int32)
    return snr, code


def decode(code, cell):
    """(time int64, width_log2) of a code map."""
    code = np.asarray(code)
    q = np.arange(code.shape[-1], dtype=np.int64) * cell
    return q + (code & 0xFFFF).astype(np.int64), code >> 16


def block_median_stats(plane, stat_block=1024):
    """(mean, var) float64 [ndm]: lower medians over the whole blocks of
    sb = min(stat_block, T) samples of the block mean and block variance."""
    x = np.asarray(plane, dtype=np.float64)
    ndm, T = x.shape
    sb = min(int(stat_block), T)
    nb = T // sb
    b = x[:, :nb * sb].reshape(ndm, nb, sb)
    m = b.sum(axis=2) / sb
    v = (b * b).sum(axis=2) / sb - m * m
    mid = (nb - 1) // 2
    return np.sort(m, axis=1)[:, mid], np.sort(v, axis=1)[:, mid]


def stats_to_f32(mean, var):
    """(mean32, rstd32) as Backend.boxcar_snr hands them to the kernel."""
    good = np.isfinite(var) & (var > 0)
    with np.errstate(all="ignore"):
        rstd = np.where(good, 1.0 / np.sqrt(np.where(good, var, 1.0)), 0.0)
    return np.asarray(mean, dtype=np.float64).astype(np.float32), rstd.astype(np.float32)


def cluster_all_pairs(j, t, w, dm_tol, time_tol):
    """Friends-of-friends labels (smallest member index) by testing all pairs."""
    j, t, w = (np.asarray(a, dtype=np.int64) for a in (j, t, w))
    n = j.size
    friends = (np.abs(j[:, None] - j[None, :]) <= dm_tol) & \
        (np.maximum(t[:, None], t[None, :]) - np.minimum((t + w)[:, None], (t + w)[None, :]) <= time_tol)
    labels = np.full(n, -1, dtype=np.int64)
    for s in range(n):
        if labels[s] >= 0:
            continue
        labels[s] = s
        stack = [s]
        while stack:
            a = stack.pop()
            for b in np.flatnonzero(friends[a] & (labels < 0)):
                labels[b] = s
                stack.append(b)
    return labels


def candidates_ref(snr, j, t, w, labels):
    """[(snr, dm_index, time, width, ncells)] one per cluster -- its maximum of
    (snr, -dm_index, -time) -- by snr descending, then (dm_index, time, width)."""
    out = []
    for lab in np.unique(labels):
        m = np.flatnonzero(labels == lab)
        b = max(m, key=lambda i: (float(snr[i]), -int(j[i]), -int(t[i])))
        out.append((float(snr[b]), int(j[b]), int(t[b]), int(w[b]), int(m.size)))
    out.sort(key=lambda c: (-c[0], c[1], c[2], c[3]))
    return out


def search_ref(plane, threshold, nw, cell, dm_tol=1, time_tol=0, stat_block=1024):
    """The whole search on the CPU with the block-median statistics: the
    candidates of candidates_ref, and the (snr, code) maps."""
    mean, var = block_median_stats(plane, stat_block)
    m32, r32 = stats_to_f32(mean, var)
    snr, code = boxcar_ref(plane, m32, r32, nw, cell)
    jj, qq = np.nonzero(snr >= np.float32(threshold))
    time, wl = decode(code, cell)
    t, w, s = time[jj, qq], 1 << wl[jj, qq].astype(np.int64), snr[jj, qq]
    labels = cluster_all_pairs(jj, t, w, dm_tol, time_tol)
    return candidates_ref(s, jj, t, w, labels), snr, code
