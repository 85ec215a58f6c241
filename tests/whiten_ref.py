"""NumPy restatement of the spectrum whitening (no GPU, no package code):

* ``plan_ref``     -- the block rule of ``Backend.whiten_plan``, integers only:
  the block at e is ``min(wmax, max(w0, e >> 3))`` bins wide and the last one
  runs to nbin once fewer than two widths are left;
* ``medians_ref``  -- ``pss_spectrum_medians`` (include/pss_hip.h): the power
  ``(re re) + (im im)`` in float32, its uint32 key (a NaN: 0xFFFFFFFF), and per
  block the key at sorted index (w - 1) // 2 -- by sorting;
* ``whiten_ref``   -- ``pss_spectrum_whiten`` in float32, one rounded operation
  per line: the norm interpolated between the doubled block centres, ``q = LN2 /
  norm``, ``s = sqrt(q)`` where 0 < norm < inf and 0 elsewhere, the product, and
  the two rules that take precedence (bins below edges[0]: (0, 0); zapped
  bins: (1, 0));
* ``zap_mask_ref`` -- the bins whose centre k df lies in a closed range.
"""
import numpy as np

LN2_F32 = np.array([0x3F317218], dtype=np.uint32).view(np.float32)[0]
NAN_KEY = np.uint32(0xFFFFFFFF)
NAN_BITS = np.uint32(0x7FC00000)


def plan_ref(nbin, kstart=1, w0=6, wmax=128):
    """edges int64 [nblk + 1]."""
    assert 1 <= w0 <= wmax <= 128 and 0 <= kstart < nbin
    edges = [kstart]
    e = kstart
    while e < nbin:
        w = min(wmax, max(w0, e >> 3))
        e = nbin if nbin - e < 2 * w else e + w
        edges.append(e)
    return np.array(edges, dtype=np.int64)


def power(spec):
    """P float32 of complex64 ``spec`` (any shape)."""
    spec = np.asarray(spec, dtype=np.complex64)
    re = np.ascontiguousarray(spec.real, dtype=np.float32)
    im = np.ascontiguousarray(spec.imag, dtype=np.float32)
    with np.errstate(all="ignore"):
        rr = re * re
        ii = im * im
        P = rr + ii
    assert P.dtype == np.float32
    return P


def medians_ref(spec, edges):
    """med float32 [ndm][nblk] of ``spec`` complex64 [ndm][nbin]."""
    P = power(spec)
    edges = np.asarray(edges, dtype=np.int64)
    key = np.where(np.isnan(P), NAN_KEY, P.view(np.uint32))
    assert key.dtype == np.uint32
    nblk = edges.size - 1
    out = np.empty((P.shape[0], nblk), dtype=np.uint32)
    for b in range(nblk):
        blk = np.sort(key[:, edges[b]:edges[b + 1]], axis=1)
        w = blk.shape[1]
        assert 1 <= w <= 256
        out[:, b] = blk[:, (w - 1) // 2]
    out[out == NAN_KEY] = NAN_BITS
    return out.view(np.float32)


def norm_ref(med, edges, nbin):
    """norm float32 [ndm][nbin]: the medians interpolated between block centres."""
    med = np.asarray(med, dtype=np.float32)
    edges = np.asarray(edges, dtype=np.int64)
    nblk = edges.size - 1
    d = edges[:-1] + edges[1:] - 1
    k2 = 2 * np.arange(nbin, dtype=np.int64)
    b = np.searchsorted(d, k2, side="right") - 1            # d_b <= 2k < d_{b+1}
    norm = np.empty((med.shape[0], nbin), dtype=np.float32)
    low = b < 0
    high = b >= nblk - 1
    mid = ~(low | high)
    norm[:, low] = med[:, :1]
    norm[:, high] = med[:, nblk - 1:]
    if mid.any():
        bm = b[mid]
        num = (k2[mid] - d[bm]).astype(np.float32)
        den = (d[bm + 1] - d[bm]).astype(np.float32)
        assert np.array_equal(num.astype(np.int64), k2[mid] - d[bm])       # (both conversions exact)
        assert np.array_equal(den.astype(np.int64), d[bm + 1] - d[bm])
        with np.errstate(all="ignore"):
            f = num / den
            diff = med[:, bm + 1] - med[:, bm]
            t = diff * f[None, :]
            nm = med[:, bm] + t
        assert f.dtype == np.float32 and diff.dtype == np.float32 and t.dtype == np.float32
        assert nm.dtype == np.float32
        norm[:, mid] = nm
    return norm


def whiten_ref(spec, edges, med=None, zap=None):
    """out complex64 [ndm][nbin] of ``spec`` complex64 [ndm][nbin] (the usable
    bins only); ``med`` defaults to ``medians_ref(spec, edges)``."""
    spec = np.asarray(spec, dtype=np.complex64)
    edges = np.asarray(edges, dtype=np.int64)
    ndm, nbin = spec.shape
    assert edges[-1] == nbin
    if med is None:
        med = medians_ref(spec, edges)
    norm = norm_ref(med, edges, nbin)
    re = np.ascontiguousarray(spec.real, dtype=np.float32)
    im = np.ascontiguousarray(spec.imag, dtype=np.float32)
    with np.errstate(all="ignore"):
        q = LN2_F32 / norm
        assert q.dtype == np.float32
        good = (norm > 0) & (norm < np.inf)
        s = np.where(good, np.sqrt(np.where(good, q, np.float32(0))), np.float32(0))
        assert s.dtype == np.float32
        ore = re * s
        oim = im * s
    assert ore.dtype == np.float32 and oim.dtype == np.float32
    if zap is not None:
        z = np.asarray(zap)[:nbin] != 0
        ore[:, z] = 1.0
        oim[:, z] = 0.0
    ore[:, :edges[0]] = 0.0
    oim[:, :edges[0]] = 0.0
    out = np.empty((ndm, nbin), dtype=np.complex64)
    out.real = ore
    out.imag = oim
    return out


def zap_mask_ref(nfft, samprate_hz, ranges):
    """uint8 [nfft // 2]: 1 where lo <= k df <= hi for a (lo, hi) of ``ranges`` (Hz), df = samprate / nfft."""
    nbin = nfft // 2
    df = float(samprate_hz) / nfft
    mask = np.zeros(nbin, dtype=np.uint8)
    for k in range(nbin):
        c = k * df
        for lo, hi in ranges:
            if lo <= c <= hi:
                mask[k] = 1
    return mask
