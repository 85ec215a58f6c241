"""NumPy restatement of the periodicity search (no GPU, no package code):

* ``harmonic_ref``   -- ``pss_harmonic_search`` (include/pss_hip.h) in float32,
  one rounded operation per line: the power ``((re re) + (im im)) scale``, the
  harmonic sums from the top ``H = H + P[(k m + h/2) / h]`` for odd m in rising
  order level by level, ``z = (H - h) a_l`` and per cell the lexicographic
  maximum of (z, -l, -k) over the valid (l, k);
* ``scale_f32``      -- the normalisation ``Backend.harmonic_snr`` hands to the
  kernel;
* ``cluster_all_pairs`` / ``candidates_ref`` -- friends-of-friends on the
  fundamental in sixteenths of a bin by testing every pair, and the candidate
  of each cluster;
* ``fft_length_ref`` -- the largest even 5-smooth length by brute force.
"""
import numpy as np

SQRT2_F32 = np.array([0x3FB504F3], dtype=np.uint32).view(np.float32)[0]


def coef(l):
    """a_l = 2^-ceil(l/2) * (l odd ? float32(sqrt 2) : 1), exact in float32."""
    s = SQRT2_F32 if l & 1 else np.float32(1.0)
    return np.float32(np.ldexp(np.float64(s), -((l + 1) // 2)))


def power(row, scale):
    """P float32 [nbin] of one complex64 row."""
    re = np.ascontiguousarray(row.real, dtype=np.float32)
    im = np.ascontiguousarray(row.imag, dtype=np.float32)
    with np.errstate(all="ignore"):
        rr = re * re
        ii = im * im
        s = rr + ii
        P = s * np.float32(scale)
    assert P.dtype == np.float32
    return P


def best_per_bin(row, scale, nl, kmin):
    """(z, l) float32 / int32 [nbin]: per bin k the largest z_l[k] over the
    valid levels, the lower level on ties; -inf, 0 where nothing beat -inf."""
    P = power(row, scale)
    nbin = P.size
    k = np.arange(nbin, dtype=np.int64)
    bz = np.full(nbin, -np.inf, dtype=np.float32)
    bl = np.zeros(nbin, dtype=np.int32)
    H = P
    with np.errstate(all="ignore"):
        for l in range(nl):
            h = 1 << l
            for m in range(1, h, 2):
                H = H + P[(k * m + h // 2) // h]
            assert H.dtype == np.float32
            d = H - np.float32(h)
            z = d * coef(l)
            assert z.dtype == np.float32
            valid = (k + h // 2) // h >= kmin
            upd = valid & (z > bz)                       # (a NaN never compares greater)
            bz[upd] = z[upd]
            bl[upd] = l
    return bz, bl


def harmonic_ref(spec, scale, nl, kmin, cell):
    """snr float32 [ndm][nq], code int32 [ndm][nq] of pss_harmonic_search;
    ``spec`` complex64 [ndm][nbin] (the usable bins only)."""
    spec = np.asarray(spec, dtype=np.complex64)
    ndm, nbin = spec.shape
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float32), (ndm,))
    nq = -(-nbin // cell)
    snr = np.full((ndm, nq), -np.inf, dtype=np.float32)
    code = np.zeros((ndm, nq), dtype=np.int32)
    koff = np.arange(nq * cell, dtype=np.int64).reshape(nq, cell) % cell
    for j in range(ndm):
        bz, bl = best_per_bin(spec[j], scale[j], nl, kmin)
        z = np.full(nq * cell, -np.inf, dtype=np.float32)
        z[:nbin] = bz
        ll = np.zeros(nq * cell, dtype=np.int64)
        ll[:nbin] = bl
        z, ll = z.reshape(nq, cell), ll.reshape(nq, cell)
        top = z.max(axis=1)                              # (no NaN is ever stored)
        key = np.where(z == top[:, None], (ll << 16) | koff, np.int64(1) << 40)
        pos = key.argmin(axis=1)                         # lower level, then lower bin
        snr[j] = z[np.arange(nq), pos]                   # the winner's own bits (-0.0 stays -0.0)
        code[j] = np.where(top == -np.inf, 0, key[np.arange(nq), pos]).astype(np.int32)
    return snr, code


def decode(code, cell):
    """(bin int64, level) of a code map."""
    code = np.asarray(code)
    q = np.arange(code.shape[-1], dtype=np.int64) * cell
    return q + (code & 0xFFFF).astype(np.int64), code >> 16


def scale_f32(var, n_used):
    """float32(1 / (var n)) in float64, 0 where var is not positive and finite."""
    var = np.asarray(var, dtype=np.float64)
    good = np.isfinite(var) & (var > 0)
    with np.errstate(all="ignore"):
        s = np.where(good, 1.0 / (np.where(good, var, 1.0) * n_used), 0.0)
    return s.astype(np.float32)


def cluster_all_pairs(j, F, dm_tol, tol16):
    """Friends-of-friends labels (smallest member index) by testing all pairs:
    friends iff |j_a - j_b| <= dm_tol and |F_a - F_b| <= tol16 (sixteenths)."""
    j, F = (np.asarray(a, dtype=np.int64) for a in (j, F))
    n = j.size
    friends = (np.abs(j[:, None] - j[None, :]) <= dm_tol) & (np.abs(F[:, None] - F[None, :]) <= tol16)
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


def candidates_ref(snr, j, k, lev, dm_tol=1, freq_tol=1.0):
    """[(snr, dm_index, bin, nharm, ncells)] one per cluster -- its maximum of
    (snr, -dm_index, -bin) -- by snr descending, then (dm_index, bin, nharm)."""
    j, k, lev = (np.asarray(a, dtype=np.int64) for a in (j, k, lev))
    labels = cluster_all_pairs(j, k << (4 - lev), dm_tol, int(round(16 * freq_tol)))
    out = []
    for lab in np.unique(labels):
        m = np.flatnonzero(labels == lab)
        b = max(m, key=lambda i: (float(snr[i]), -int(j[i]), -int(k[i])))
        out.append((float(snr[b]), int(j[b]), int(k[b]), 1 << int(lev[b]), int(m.size)))
    out.sort(key=lambda c: (-c[0], c[1], c[2], c[3]))
    return out


def search_ref(spec, scale, threshold, nl, kmin, cell, dm_tol=1, freq_tol=1.0):
    """The search of a spectrum [ndm][nbin] on the CPU: the candidates of
    candidates_ref, and the (snr, code) maps."""
    snr, code = harmonic_ref(spec, scale, nl, kmin, cell)
    jj, qq = np.nonzero(snr >= np.float32(threshold))
    k, lev = decode(code, cell)
    return candidates_ref(snr[jj, qq], jj, k[jj, qq], lev[jj, qq], dm_tol, freq_tol), snr, code


def fft_length_ref(T):
    """The largest even n <= T with no prime factor above 5, by trial division."""
    for n in range(T - (T % 2), 1, -2):
        r = n
        for p in (2, 3, 5):
            while r % p == 0:
                r //= p
        if r == 1:
            return n
    raise ValueError(T)
