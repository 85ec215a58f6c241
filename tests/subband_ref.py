"""Float64 oracle of the sub-band dedispersion (``Backend.subband_plan`` /
``subband_dedisperse``) and of the banded entry ``pss_dedisperse_banded``, as
plain loops of slices.  Nothing here touches a device."""
import numpy as np


def direct(data, table, max_delay):
    """out[j][t] = sum_c data[c][t + clip(table[j][c], 0, max_delay)], t < N - max_delay."""
    data = np.asarray(data, dtype=np.float64)
    d = np.clip(np.asarray(table, dtype=np.int64), 0, max_delay)
    T = data.shape[1] - max_delay
    out = np.zeros((d.shape[0], T))
    for j in range(d.shape[0]):
        for c in range(d.shape[1]):
            out[j] += data[c, d[j, c]:d[j, c] + T]
    return out


def banded(planes, table, per_src, max_delay, band):
    """pss_dedisperse_banded: ``planes`` [nsrc][nchan][n] -> out [ndm][nb][T]."""
    planes = np.asarray(planes, dtype=np.float64)
    nsrc, nchan, n = planes.shape
    d = np.clip(np.asarray(table, dtype=np.int64), 0, max_delay)
    ndm = d.shape[0]
    nb = -(-nchan // band)
    T = n - max_delay
    out = np.zeros((ndm, nb, T))
    for j in range(ndm):
        q = min(j // per_src, nsrc - 1)
        for s in range(nb):
            for c in range(s * band, min(nchan, (s + 1) * band)):
                out[j, s] += planes[q, c, d[j, c]:d[j, c] + T]
    return out


def plan(D, freqs, nsub, group, N):
    """The tables of section 1 from the exact table D [nDM][C], one scalar at a
    time: dict(ref, nominal, d1, d2, e, m1, m2, T1, T)."""
    D = np.asarray(D, dtype=np.int64)
    ndm, C = D.shape
    band = C // nsub
    ref = []
    for s in range(nsub):
        r = s * band
        for c in range(s * band, (s + 1) * band):
            if freqs[c] > freqs[r]:
                r = c
        ref.append(r)
    ngroups = -(-ndm // group)
    nominal = [(g * group + min(ndm, (g + 1) * group) - 1) // 2 for g in range(ngroups)]
    d1 = np.zeros((ngroups, C), dtype=np.int64)
    d2 = np.zeros((ndm, nsub), dtype=np.int64)
    e = np.zeros((ndm, C), dtype=np.int64)
    for g in range(ngroups):
        for c in range(C):
            d1[g, c] = D[nominal[g], c] - D[nominal[g], ref[c // band]]
    for j in range(ndm):
        for s in range(nsub):
            d2[j, s] = D[j, ref[s]]
        for c in range(C):
            e[j, c] = d1[j // group, c] + d2[j, c // band]
    m1, m2 = int(d1.max()), int(d2.max())
    return dict(ref=np.array(ref), nominal=np.array(nominal), d1=d1, d2=d2, e=e, m1=m1, m2=m2, T1=N - m1,
                T=N - m1 - m2)


def two_stage(data, p, nsub, group):
    """plane [nDM][T] of section 1 from the tables ``p`` of :func:`plan`, stage by stage."""
    data = np.asarray(data, dtype=np.float64)
    C = data.shape[0]
    band = C // nsub
    ngroups, ndm = p["d1"].shape[0], p["d2"].shape[0]
    sub = np.zeros((ngroups, nsub, p["T1"]))
    for g in range(ngroups):
        for c in range(C):
            sub[g, c // band] += data[c, p["d1"][g, c]:p["d1"][g, c] + p["T1"]]
    out = np.zeros((ndm, p["T"]))
    for j in range(ndm):
        for s in range(nsub):
            out[j] += sub[j // group, s, p["d2"][j, s]:p["d2"][j, s] + p["T"]]
    return out


def banded_good(data, delays, out):
    """Valid arguments of pss_dedisperse_banded by name, in call order (the trailing stream is NULL)."""
    # pss_dedisperse_banded(data, nsrc, src_stride, nchan, n, ld, delays, ndm, per_src, max_delay, band, out, out_ld)
    return dict(data=data, nsrc=2, src_stride=400, nchan=4, n=100, ld=100, delays=delays, ndm=3, per_src=2,
                max_delay=10, band=2, out=out, out_ld=90)


# (overrides, word of the error) -- every PSS_EINVAL case of the entry
BANDED_REJECTIONS = ((dict(data=None), "data"), (dict(delays=None), "delays"), (dict(out=None), "out"),
                     (dict(nsrc=0), "nsrc 0"), (dict(nsrc=-1), "nsrc -1"),
                     (dict(nchan=0, src_stride=0), "nchan 0"), (dict(nchan=-3), "nchan -3"),
                     (dict(ndm=0), "ndm 0"), (dict(ndm=-1), "ndm -1"),
                     (dict(per_src=0), "per_src 0"), (dict(per_src=-5), "per_src -5"),
                     (dict(band=0), "band 0"), (dict(band=-2), "band -2"),
                     (dict(ld=99), "ld 99"),
                     (dict(src_stride=399), "src_stride 399"), (dict(src_stride=399, nsrc=1), "src_stride 399"),
                     (dict(src_stride=-1), "src_stride -1"),
                     (dict(max_delay=-1), "max_delay -1"),
                     (dict(max_delay=100), "max_delay 100"), (dict(max_delay=101, out_ld=0), "max_delay 101"),
                     (dict(n=0, ld=0, max_delay=0), "max_delay 0 >= n 0"),
                     (dict(out_ld=89), "out_ld 89"), (dict(max_delay=0, out_ld=99), "out_ld 99"),
                     # the launch grid: ceil(T / 2048) * bands * trial groups in 31 bits
                     (dict(n=1 << 40, ld=1 << 40, src_stride=1 << 42, out_ld=1 << 40, ndm=64, per_src=64),
                      "workgroups"),
                     (dict(n=1 << 36, ld=1 << 36, src_stride=1 << 48, out_ld=1 << 36, nchan=4096, band=1),
                      "workgroups"),
                     (dict(n=1 << 30, ld=1 << 30, src_stride=1 << 42, out_ld=1 << 30, nchan=4096, band=4, ndm=1 << 14,
                           per_src=1), "workgroups"))
