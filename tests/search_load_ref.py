"""What the search-mode loader's tests share: a float64 NumPy restatement of
``pss_unpack_tmajor`` with its error bound, the packing of codes into bytes,
and a host writer of search-mode PSRFITS files with layouts the package's own
writer never produces (several polarisations, a descending band, weights,
ZERO_OFF), composed from the package's card and header helpers.

The restatement (include/pss_hip.h), codes [nrows][nsblk][npol][nchan]:

    v_p = (code - zero_off) * scl[r][p][c] + offs[r][p][c]          p < nsum
    x   = (sum_p v_p) * w[r][c]
    out[flip ? nchan-1-c : c][r nsblk + t] = x

The bound.  The kernel rounds at most four times on any path (the subtraction
of zero_off, the fused multiply-add, the sum of the two polarisations, the
weight), each by a relative 2^-24 of a magnitude no larger than
M = sum_p (|code - zero_off| |scl_p| + |offs_p|); compounding four factors
(1 + 2^-24) adds less than 2^-20 of that:

    |got - ref64| <= 4 2^-24 (1 + 2^-20) |w| M
"""
import numpy as np

from psrsigsim_amd.io.psrfits import _card, _header

EPS = 4.0 * 2.0 ** -24 * (1.0 + 2.0 ** -20)


def pack(codes, nbits):
    """codes [..., nchan] -> bytes [..., nchan nbits / 8]: the lower-numbered
    channel in the more significant bits of its byte."""
    c = np.asarray(codes).astype(np.uint8)
    if nbits == 8:
        return c
    if nbits == 4:
        return (c[..., 0::2] << 4) | c[..., 1::2]
    return (c[..., 0::4] << 6) | (c[..., 1::4] << 4) | (c[..., 2::4] << 2) | c[..., 3::4]


def unpack_ref(codes, scl, offs, wts=None, zero_off=0.0, nsum=1, flip=False):
    """(ref, bound), float64 [nchan][nrows nsblk].  codes [nrows][nsblk][npol]
    [nchan]; scl / offs [nrows][npol][nchan]; wts [nrows][nchan] or None."""
    nrows, nsblk, npol, nchan = codes.shape
    u = codes[:, :, :nsum, :].astype(np.float64) - float(zero_off)
    s = np.asarray(scl, dtype=np.float64).reshape(nrows, 1, npol, nchan)[:, :, :nsum]
    o = np.asarray(offs, dtype=np.float64).reshape(nrows, 1, npol, nchan)[:, :, :nsum]
    w = np.ones((nrows, nchan)) if wts is None else np.asarray(wts, dtype=np.float64).reshape(nrows, nchan)
    ref = (u * s + o).sum(axis=2) * w[:, None, :]
    bound = EPS * np.abs(w[:, None, :]) * (np.abs(u) * np.abs(s) + np.abs(o)).sum(axis=2)
    tmajor = lambda a: np.ascontiguousarray(a.reshape(nrows * nsblk, nchan).T[::-1 if flip else 1])
    return tmajor(ref), tmajor(bound)


def write_search_file(path, codes, scl, offs, wts, freq, nbits, pol_type="AA+BB", zero_off=0.0, tbin=64e-6,
                      obsfreq=1400.0, obsbw=400.0, dm=None, cards=()):
    """A search-mode PSRFITS file of the given codes [nrows][nsblk][npol]
    [nchan], DAT_SCL / DAT_OFFS [nrows][npol][nchan], DAT_WTS [nrows][nchan]
    and DAT_FREQ [nchan] (or [nrows][nchan]), packed with NumPy.  ``cards``:
    (key, value) pairs that replace or extend the SUBINT header's (NBITS,
    SIGNINT, NBIN .. for the files a loader must refuse)."""
    codes = np.asarray(codes)
    nrows, nsblk, npol, nchan = codes.shape
    nb = nchan * nbits // 8
    packed = pack(codes, nbits).reshape(nrows, nsblk * npol * nb)
    row = np.dtype([("TSUBINT", ">f8"), ("OFFS_SUB", ">f8"), ("DAT_FREQ", ">f8", (nchan,)),
                    ("DAT_WTS", ">f4", (nchan,)), ("DAT_OFFS", ">f4", (npol * nchan,)),
                    ("DAT_SCL", ">f4", (npol * nchan,)), ("DATA", "u1", (nsblk * npol * nb,))])
    tab = np.zeros(nrows, dtype=row)
    tab["TSUBINT"] = nsblk * tbin
    tab["OFFS_SUB"] = (np.arange(nrows) + 0.5) * nsblk * tbin
    tab["DAT_FREQ"] = freq
    tab["DAT_WTS"] = wts
    tab["DAT_OFFS"] = np.asarray(offs, dtype=np.float32).reshape(nrows, npol * nchan)
    tab["DAT_SCL"] = np.asarray(scl, dtype=np.float32).reshape(nrows, npol * nchan)
    tab["DATA"] = packed
    prim = [_card("SIMPLE", True), _card("BITPIX", 8), _card("NAXIS", 0), _card("EXTEND", True),
            _card("FITSTYPE", "PSRFITS"), _card("OBS_MODE", "SEARCH"), _card("OBSFREQ", float(obsfreq)),
            _card("OBSBW", float(obsbw)), _card("OBSNCHAN", nchan)]
    sub = {"XTENSION": "BINTABLE", "BITPIX": 8, "NAXIS": 2, "NAXIS1": row.itemsize, "NAXIS2": nrows, "PCOUNT": 0,
           "GCOUNT": 1, "TFIELDS": 7}
    forms = [("TSUBINT", "1D"), ("OFFS_SUB", "1D"), ("DAT_FREQ", "%dD" % nchan), ("DAT_WTS", "%dE" % nchan),
             ("DAT_OFFS", "%dE" % (npol * nchan)), ("DAT_SCL", "%dE" % (npol * nchan)),
             ("DATA", "%dB" % (nsblk * npol * nb))]
    for i, (name, form) in enumerate(forms, 1):
        sub["TTYPE%d" % i] = name
        sub["TFORM%d" % i] = form
    sub["TDIM7"] = "(1,%d,%d,%d)" % (nb, npol, nsblk)
    sub.update({"EXTNAME": "SUBINT", "INT_TYPE": "TIME", "NPOL": npol, "POL_TYPE": pol_type, "TBIN": float(tbin),
                "NBIN": 1, "NCHAN": nchan, "CHAN_BW": float(obsbw) / nchan, "NSBLK": nsblk, "NBITS": nbits,
                "ZERO_OFF": float(zero_off), "SIGNINT": 0, "NSUBOFFS": 0})
    if dm is not None:
        sub["DM"] = float(dm)
    sub.update(dict(cards))
    body = tab.tobytes()
    with open(path, "wb") as f:
        f.write(_header(prim))
        f.write(_header([_card(k, v) for k, v in sub.items()]))
        f.write(body + b"\0" * ((-len(body)) % 2880))


def random_case(nbits, nchan, nsblk, nrows, npol=1, nsum=1, seed=0):
    """Uniform random codes and float32 scl / offs of either sign.  The
    polarisations at or beyond ``nsum`` get scales and offsets 1e6 times
    larger: a kernel that read them would miss every bound."""
    rng = np.random.default_rng(7000 + seed + 100 * nbits + 10 * nchan + nsblk)
    codes = rng.integers(0, 1 << nbits, (nrows, nsblk, npol, nchan), dtype=np.uint8)
    scl = rng.uniform(0.25, 4.0, (nrows, npol, nchan)) * rng.choice([-1.0, 1.0], (nrows, npol, nchan))
    offs = rng.normal(0.0, 50.0, (nrows, npol, nchan))
    scl[:, nsum:] *= 1e6
    offs[:, nsum:] *= 1e6
    return codes, scl.astype(np.float32), offs.astype(np.float32)
