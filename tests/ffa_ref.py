"""NumPy restatement of the fast folding search (no GPU, no package code):

* ``scrunch_ref``   -- ``pss_ffa_scrunch`` (include/pss_hip.h): the pairwise
  tree ``y = y[0::2] + y[1::2]`` level by level, in float32;
* ``transform_block`` / ``transform_ref`` -- ``pss_ffa_transform``: the
  top-down halving recursion, one float32 add per output sample;
* ``profile_search_ref`` -- ``pss_ffa_profile_search``: the circular boxcar
  tree, ``z = (S * a_k) * g`` with ``g = rstd * rm`` one rounded product, and
  per cell the lexicographic maximum of (z, -k, -s, -phase);
* ``decode``, ``plan_ref`` (the octave plan of ``Backend.ffa_plan``),
  ``snr_ref`` (``Backend.ffa_snr``, the maps of every octave in plan order) and
  ``search_ref`` (with ``pulse_search_ref.block_median_stats``, clustered by
  testing all pairs).
"""
import math

import numpy as np

from tests import pulse_search_ref as psr

LDS_FLOATS = 8192                    # kFfaLds of pss_ffa.hip: floats of a subtree the kernel keeps in LDS


def scrunch_ref(x, lf, sub=None):
    """y float32 [nser][T >> lf]."""
    x = np.asarray(x, dtype=np.float32)
    nser, T = x.shape
    n = T >> lf
    y = x[:, :n << lf]
    with np.errstate(all="ignore"):
        if sub is not None:
            y = y - np.broadcast_to(np.asarray(sub, dtype=np.float32), (nser,))[:, None]
        for _ in range(lf):
            y = y[:, 0::2] + y[:, 1::2]
    assert y.dtype == np.float32 and y.shape == (nser, n)
    return np.array(y)


def rule(m):
    """(i_s, j_s, b_s) int64 [m] of a node of m >= 2 rows."""
    h = m // 2
    t = m - h
    s = np.arange(m, dtype=np.int64)
    den = 2 * (m - 1)
    return (2 * s * (h - 1) + (m - 1)) // den, (2 * s * (t - 1) + (m - 1)) // den, (2 * s * h + (m - 1)) // den


def transform_block(rows):
    """F(0, m) float32 [m][p] of the leaves ``rows`` [m][p]."""
    rows = np.asarray(rows, dtype=np.float32)
    m, p = rows.shape
    if m == 1:
        return rows.copy()
    h = m // 2
    H = transform_block(rows[:h])
    Tl = transform_block(rows[h:])
    i, j, b = rule(m)
    idx = (np.arange(p, dtype=np.int64)[None, :] + b[:, None]) % p
    with np.errstate(all="ignore"):
        out = H[i] + Tl[j[:, None], idx]
    assert out.dtype == np.float32
    return out


def transform_ref(y, p0, np_, fill=np.nan):
    """out float32 [nser][np][n]; words [m p, n) of a block hold ``fill``."""
    y = np.asarray(y, dtype=np.float32)
    nser, n = y.shape
    out = np.full((nser, np_, n), fill, dtype=np.float32)
    for i in range(nser):
        for pi in range(np_):
            p = p0 + pi
            m = n // p
            out[i, pi, :m * p] = transform_block(y[i, :m * p].reshape(m, p)).reshape(-1)
    return out


def depth(m):
    """ceil(log2 m)."""
    return (m - 1).bit_length()


def fuse_depth(m, p):
    """The depth below which pss_ffa_transform computes a subtree in LDS."""
    d = 0
    while ((m + (1 << d) - 1) >> d) * p > LDS_FLOATS:
        d += 1
    return d


def best_per_profile(prof, g, nw):
    """(z float32, k, phase int64) [m]: the lexicographic maximum of (z, -k,
    -phase) of every profile of ``prof`` [m][p]; -inf, 0, 0 where nothing beat -inf."""
    prof = np.asarray(prof, dtype=np.float32)
    m, p = prof.shape
    g = np.float32(g)
    bz = np.full((m, p), -np.inf, dtype=np.float32)
    bk = np.zeros((m, p), dtype=np.int64)
    S = prof
    with np.errstate(all="ignore"):
        for k in range(nw):
            if (2 << k) > p:
                break
            w = S * psr.coef(k)
            z = w * g
            assert z.dtype == np.float32
            upd = z > bz                                   # (a NaN never compares greater; k rises: ties stay)
            bz[upd] = z[upd]
            bk[upd] = k
            S = S + np.roll(S, -(1 << k), axis=1)
    top = bz.max(axis=1)
    key = np.where(bz == top[:, None], (bk << 16) | np.arange(p, dtype=np.int64)[None, :], np.int64(1) << 40)
    pos = key.argmin(axis=1)
    r = np.arange(m)
    none = top == -np.inf
    return bz[r, pos], np.where(none, 0, bk[r, pos]), np.where(none, 0, pos)


def profile_search_ref(prof, n, p0, np_, rstd, rm, nw, cell):
    """(snr float32, code int32, phase int32) [nser][np][nq] of
    pss_ffa_profile_search on ``prof`` [nser][np][n]."""
    prof = np.asarray(prof, dtype=np.float32)
    nser = prof.shape[0]
    rstd = np.broadcast_to(np.asarray(rstd, dtype=np.float32), (nser,))
    rm = np.broadcast_to(np.asarray(rm, dtype=np.float32), (np_,))
    nq = -(-(n // p0) // cell)
    snr = np.full((nser, np_, nq), -np.inf, dtype=np.float32)
    code = np.zeros((nser, np_, nq), dtype=np.int32)
    phase = np.zeros((nser, np_, nq), dtype=np.int32)
    for i in range(nser):
        for pi in range(np_):
            p = p0 + pi
            m = n // p
            with np.errstate(all="ignore"):
                g = np.float32(rstd[i] * rm[pi])
            z, k, f = best_per_profile(prof[i, pi, :m * p].reshape(m, p), g, nw)
            for q in range(-(-m // cell)):
                s0, s1 = q * cell, min((q + 1) * cell, m)
                zz = z[s0:s1]
                top = zz.max()
                if top == -np.inf:
                    continue
                key = np.where(zz == top, (k[s0:s1] << 32) | (np.arange(s1 - s0, dtype=np.int64) << 16) | f[s0:s1],
                               np.int64(1) << 60)
                b = int(key.argmin())
                snr[i, pi, q] = zz[b]
                code[i, pi, q] = (int(k[s0 + b]) << 16) | b
                phase[i, pi, q] = f[s0 + b]
    return snr, code, phase


def decode(code, cell):
    """(shift int64, width_log2) of a code map whose last axis runs over the cells."""
    code = np.asarray(code)
    q = np.arange(code.shape[-1], dtype=np.int64) * cell
    return q + (code & 0xFFFF).astype(np.int64), code >> 16


def plan_ref(T, fs, pmin, pmax, bins=256):
    """The octaves of Backend.ffa_plan as (lf, n, p0, np) tuples."""
    B = int(bins)
    a, b = float(pmin) * float(fs), float(pmax) * float(fs)
    assert B <= a <= b
    lf = int(math.floor(math.log2(a / B)))
    while B * 2.0 ** (lf + 1) <= a:                        # (the logarithm's rounding, either way)
        lf += 1
    while B * 2.0 ** lf > a:
        lf -= 1
    first = lf
    octs = []
    while B * 2.0 ** lf <= b:
        n = int(T) >> lf
        p0 = max(B, int(math.floor(a / 2.0 ** lf))) if lf == first else B
        pl = min(2 * B - 1, int(math.ceil(b / 2.0 ** lf)))
        assert n // pl >= 2
        octs.append((lf, n, p0, pl - p0 + 1))
        lf += 1
    return octs


def snr_ref(plane, fs, pmin, pmax, mean32, rstd32, bins=256, nw=6, cell=16):
    """The maps of Backend.ffa_snr: dict of snr float32, code, phase int32,
    shift, width_log2 int64, period float64 [ndm][ncols] and the column table
    (octave, lf, p, m, q) int64 [ncols][5], every (octave, base period, cell) in plan order."""
    plane = np.asarray(plane, dtype=np.float32)
    ndm, T = plane.shape
    maps = {k: [] for k in ("snr", "code", "phase", "shift", "period")}
    cols = []
    for o, (lf, n, p0, np_) in enumerate(plan_ref(T, fs, pmin, pmax, bins)):
        y = scrunch_ref(plane, lf, mean32)
        prof = transform_ref(y, p0, np_)
        ms = [n // (p0 + pi) for pi in range(np_)]
        rm = np.array([1.0 / math.sqrt(m * 2.0 ** lf) for m in ms]).astype(np.float32)
        snr, code, phase = profile_search_ref(prof, n, p0, np_, rstd32, rm, nw, cell)
        shift, _ = decode(code, cell)
        for pi in range(np_):
            p, m = p0 + pi, ms[pi]
            nqp = -(-m // cell)
            maps["snr"].append(snr[:, pi, :nqp])
            maps["code"].append(code[:, pi, :nqp])
            maps["phase"].append(phase[:, pi, :nqp])
            maps["shift"].append(shift[:, pi, :nqp])
            maps["period"].append((p + shift[:, pi, :nqp].astype(np.float64) / (m - 1)) * 2.0 ** lf / float(fs))
            cols += [(o, lf, p, m, q) for q in range(nqp)]
    out = {k: np.concatenate(v, axis=1) for k, v in maps.items()}
    out["width_log2"] = (out["code"] >> 16).astype(np.int64)
    out["columns"] = np.array(cols, dtype=np.int64)
    return out


def candidates_ref(maps, T, fs, threshold, dm_tol=1, freq_tol=1.0):
    """[(snr, dm_index, period, width, phase, bins, octave, shift, ncells)]: the
    cells at or above the threshold clustered on (trial, F = round(16 T /
    P_samples)) by testing all pairs, one candidate per cluster -- its maximum
    of (snr, -dm_index, -F) -- by snr descending, then (dm_index, period)."""
    jj, cc = np.nonzero(maps["snr"] >= np.float32(threshold))
    s = maps["snr"][jj, cc]
    per = maps["period"][jj, cc]
    F = np.rint(16.0 * T / (per * float(fs))).astype(np.int64)
    labels = psr.cluster_all_pairs(jj, F, np.zeros_like(F), dm_tol, int(round(16 * float(freq_tol))))
    out = []
    for lab in np.unique(labels):
        mem = np.flatnonzero(labels == lab)
        b = max(mem, key=lambda i: (float(s[i]), -int(jj[i]), -int(F[i])))
        c = cc[b]
        out.append((float(s[b]), int(jj[b]), float(per[b]), 1 << int(maps["width_log2"][jj[b], c]),
                    int(maps["phase"][jj[b], c]), int(maps["columns"][c, 2]), int(maps["columns"][c, 0]),
                    int(maps["shift"][jj[b], c]), int(mem.size)))
    out.sort(key=lambda c: (-c[0], c[1], c[2]))
    return out


def search_ref(plane, fs, pmin, pmax, threshold, bins=256, nw=6, cell=16, dm_tol=1, freq_tol=1.0, stat_block=1024):
    """The whole search on the CPU with the block-median statistics: the
    candidates of candidates_ref and the maps of snr_ref."""
    mean, var = psr.block_median_stats(plane, stat_block)
    m32, r32 = psr.stats_to_f32(mean, var)
    maps = snr_ref(plane, fs, pmin, pmax, m32, r32, bins, nw, cell)
    return candidates_ref(maps, np.asarray(plane).shape[1], fs, threshold, dm_tol, freq_tol), maps
