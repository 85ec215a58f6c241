"""NumPy restatement of the candidate fold (``pss_fold_series``,
``Backend.fold_candidates``, ``FoldedCandidates.refine``): the oracle of
tests/test_fold_candidates_host.py and tests/test_gpu_fold_candidates.py.
Nothing here imports the package.

Phases are 64-bit fixed point with wrapping uint64 arithmetic:

    inc    = floor(2^64 / Ps + 1/2)          Ps the period in samples, an exact rational
    phi(u) = (phi0 + u inc) mod 2^64
    bin(u) = ((phi(u) >> 32) nbin) >> 32
"""
from fractions import Fraction

import numpy as np

DM_K = 1.0 / 2.41e-4           # psrsigsim_amd.utils.constants.DM_K_VALUE (s MHz^2 cm^3 / pc)
MASK = (1 << 64) - 1


def phase_step(period_samples):
    q = Fraction(1 << 64) / Fraction(float(period_samples)) + Fraction(1, 2)
    return q.numerator // q.denominator


def inc_limit(nbin):
    return (1 << 64) // int(nbin)


def bins(n, inc, phi0, nbin, u0=0):
    """bin(u) for u0 <= u < u0 + n (int64 array)."""
    with np.errstate(over="ignore"):
        u = np.arange(u0, u0 + n, dtype=np.uint64)
        phi = np.uint64(phi0 & MASK) + u * np.uint64(inc & MASK)
        return (((phi >> np.uint64(32)) * np.uint64(nbin)) >> np.uint64(32)).astype(np.int64)


def fold_series(x, src, inc, phi0, nsub, L, nbin):
    """(out float64 [nrows][nsub][nbin] -- not yet rounded to float32 --, hits
    int64, mag = the same sums over |x|) of pss_fold_series, clamps included."""
    x = np.asarray(x, dtype=np.float64)
    nser = x.shape[0]
    nrows = len(src)
    out = np.zeros((nrows, nsub, nbin))
    mag = np.zeros((nrows, nsub, nbin))
    hits = np.zeros((nrows, nsub, nbin), dtype=np.int64)
    for r in range(nrows):
        i = min(max(int(src[r]), 0), nser - 1)
        step = min(int(inc[r]), inc_limit(nbin))
        p0 = 0 if phi0 is None else int(phi0[r])
        for s in range(nsub):
            b = bins(L, step, p0, nbin, u0=s * L)
            seg = x[i, s * L:(s + 1) * L]
            out[r, s] = np.bincount(b, weights=seg, minlength=nbin)
            mag[r, s] = np.bincount(b, weights=np.abs(seg), minlength=nbin)
            hits[r, s] = np.bincount(b, minlength=nbin)
    return out, hits, mag


def roll(v, r):
    """roll(v, r)[b] = v[(b + r) mod nbin]"""
    n = len(v)
    return np.array([v[(b + r) % n] for b in range(n)], dtype=np.float64)


def drift_shift(i, s, nsub):
    return (i * (2 * s + 1) + nsub) // (2 * nsub)


def dm_bins(m, dm_step, band_w, fs_hz, Ps, nbin):
    return [int(np.floor(DM_K * m * dm_step * band_w[g] * fs_hz / Ps * nbin + 0.5)) for g in range(len(band_w))]


def chi2(p, H, M, V):
    nbin = len(p)
    if not (np.isfinite(V) and V > 0):
        return 0.0
    tot = 0.0
    for b in range(nbin):
        if H[b] > 0:
            tot += (p[b] - M * H[b]) ** 2 / (V * H[b])
    return tot / (nbin - 1)


def best(chis, n):
    order = sorted(range(-n, n + 1), key=lambda v: (abs(v), v))
    top = order[0]
    for i in order:
        if chis[i] > chis[top]:
            top = i
    return top


def refine(cube, hits, mean, var, Ps, dm, band_w, fs_hz, L, ndrift=None, ndm=None, dm_step=None):
    """One candidate: cube [nband][nsub][nbin], hits [nsub][nbin], mean / var
    [nband].  Returns a dict of the fields of FoldedCandidates.refine."""
    cube = np.asarray(cube, dtype=np.float64)
    hits = np.asarray(hits, dtype=np.float64)
    nband, nsub, nbin = cube.shape
    nd = nbin // 4 if ndrift is None else ndrift
    nm = nbin // 4 if ndm is None else ndm
    M, V = float(np.sum(mean)), float(np.sum(var))

    def aligned(i):
        B = np.zeros((nband, nbin))
        H = np.zeros(nbin)
        for s in range(nsub):
            r = drift_shift(i, s, nsub)
            H += roll(hits[s], r)
            for g in range(nband):
                B[g] += roll(cube[g, s], r)
        return B, H

    chis = {}
    for i in range(-nd, nd + 1):
        B, H = aligned(i)
        chis[i] = chi2(B.sum(axis=0), H, M, V)
    ibest = best(chis, nd)
    B, H = aligned(ibest)
    if dm_step is None:
        wmax = float(np.max(band_w))
        dm_step = Ps / (DM_K * wmax * fs_hz * nbin) if wmax > 0 else 0.0

    def summed(Bands, m):
        q = dm_bins(m, dm_step, band_w, fs_hz, Ps, nbin)
        p = np.zeros(nbin)
        for g in range(nband):
            p += roll(Bands[g], q[g])
        return p

    chim = {m: chi2(summed(B, m), H, M, V) for m in range(-nm, nm + 1)}
    mbest = best(chim, nm)
    p = summed(B, mbest)
    B0, H0 = aligned(0)
    return dict(chi2=chi2(summed(B0, 0), H0, M, V), drift=ibest,
                period_opt=1.0 / (1.0 / Ps - ibest / (float(nbin) * nsub * L)) / fs_hz, dm_shift=mbest,
                dm_opt=dm + mbest * dm_step, chi2_opt=chim[mbest], peak_bin=int(np.argmax(p)), profile=p,
                dm_step=dm_step)
