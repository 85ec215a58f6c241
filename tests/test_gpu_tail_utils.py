"""The utility kernels of csrc/pss_pipeline.hip through the C ABI, on guarded
strided rows, against float64 / exact integer references: pss_down_sample,
pss_rebin, pss_clip_cast, pss_fold, pss_fold_periods, pss_null_shift.

Inputs are ``GuardedInput`` rows (ld >= len, base on the 16-byte grid and one
float off it, every other word 2^20), outputs ``GuardedOutput``.  A launch
covers 4096 x 256 items before its grid-stride loop runs (stream_grid), so
every kernel has one case of 1 048 600 items on one row.

The means (down_sample, rebin).  Samples are k 2^-s with integer k < 2^24, so
a window's sum S 2^-s is exact in float64, on the device (a sequential float64
sum) and here (int64).  The device rounds q = fl64(S / w) to float32; the
reference is the exact mean S / w rounded ONCE.  The two can differ only where
the exact mean lies within 2^-53 (relative) of a float32 rounding midpoint; the
band asserted here is the wider (w + 2) 2^-53 that covers a float64 sum with
rounding steps too.  Outside the band: the same bits; inside: at most 1 ulp,
with the reference rounded exactly (fractions); and the test first asserts, on
its own inputs, that at most 0.1 % of the outputs lie in the band (expected:
none).  Where every window width is a power of two q is the exact mean and the
bits must agree everywhere.

The folds.  Integer samples below 2^20: float64 sums are exact integers, the
result is their float32 rounding, the same bits as NumPy's.
"""
from fractions import Fraction

import numpy as np
import pytest

from tests import kernel_harness as kh

gpu = pytest.mark.gpu            # (the reference of the means has a host test of its own below)
BIG = 1048600                 # items: just above one launch's 4096 x 256
IN_GUARD = float(1 << 20)
BAND_CAP = 1e-3


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------
# exact window means
# ---------------------------------------------------------------------------
def _round_once(S, w, s):
    """float32 nearest (ties to even) of the rational S / (w 2^s), S > 0."""
    m = Fraction(int(S), int(w) << s)
    e = 0
    while m >= 1 << 24:
        m /= 2
        e += 1
    while m < 1 << 23:
        m *= 2
        e -= 1
    n = m.numerator // m.denominator
    rem = m - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    return np.float32(np.ldexp(np.float64(n), e))


def mean_reference(k, s, lo, hi):
    """Windows [lo_i, hi_i) of the rows k 2^-s (k int64 [rows][n]): the exact
    means rounded once to float32 [rows][nwin] (NaN for an empty window), and
    the mask of the outputs inside the double-rounding band."""
    cs = np.concatenate([np.zeros((k.shape[0], 1), np.int64), np.cumsum(k, axis=1, dtype=np.int64)], axis=1)
    S = cs[:, hi] - cs[:, lo]
    w = np.broadcast_to((hi - lo).astype(np.int64), S.shape)
    assert S.max() < 1 << 53
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.ldexp(S.astype(np.float64) / w.astype(np.float64), -s)       # fl64(S / w) 2^-s: one rounding
        ref = q.astype(np.float32)
        mant, _ = np.frexp(q)
        t = mant * float(1 << 24)                                            # the float32 grid: integers
        dist = np.abs(t - np.floor(t) - 0.5) / t
    pow2 = (w & (w - 1)) == 0
    band = (w > 0) & (S > 0) & ~pow2 & (dist <= (w + 2.0) * 2.0 ** -53)
    for r, i in np.argwhere(band):
        ref[r, i] = _round_once(S[r, i], w[r, i], s)
    return ref, band


def test_mean_reference_rounds_once():
    """(host) the reference itself: exact on representable means, NaN on an
    empty window, and ties and near-ties rounded the way the exact value says."""
    k = np.array([[3, 5, 6, 2, 0, 0, 0]], dtype=np.int64)
    ref, band = mean_reference(k, 0, np.array([0, 0, 2, 0]), np.array([2, 4, 2, 3]))
    assert np.array_equal(ref[0, [0, 1]], np.float32([4.0, 4.0])) and np.isnan(ref[0, 2]) and not band.any()
    assert ref[0, 3] == np.float32(14.0 / 3.0)
    # (float32 spacing 2 above 2^24)
    assert _round_once((1 << 24) + 1, 1, 0) == np.float32(1 << 24)                # a tie: to even, downwards
    assert _round_once((1 << 24) + 3, 1, 0) == np.float32((1 << 24) + 4)          # a tie: to even, upwards
    assert _round_once(6 * ((1 << 24) + 1) + 1, 6, 0) == np.float32((1 << 24) + 2)   # a sixth above a tie
    assert _round_once(6 * ((1 << 24) + 1) - 1, 6, 0) == np.float32(1 << 24)         # a sixth below it
    k = np.array([[6 * ((1 << 24) + 1) - 1, 0, 0, 0, 0, 0]], dtype=np.int64)      # (far outside the band)
    ref, band = mean_reference(k, 0, np.array([0]), np.array([6]))
    assert ref[0, 0] == np.float32(1 << 24) and not band.any()
    assert _round_once(1, 3, 24) == np.float32(2.0 ** -24 / 3)


def _sample_sets(rows, n, seed):
    """(name, k int64 [rows][n], s): the rows are k 2^-s, exact in float32."""
    rng = np.random.default_rng(seed)
    yield "integers", rng.integers(0, 1 << 20, (rows, n), dtype=np.int64), 0
    yield "uniform", rng.integers(0, 1 << 24, (rows, n), dtype=np.int64), 24


def _check_means(got, ref, band, what):
    frac = band.mean()
    print("%s: band fraction %.3g (%d of %d)" % (what, frac, int(band.sum()), band.size))
    assert frac <= BAND_CAP, what
    g, r = got.view(np.int32).astype(np.int64), ref.view(np.int32).astype(np.int64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    assert np.array_equal(g[~band & ~nan], r[~band & ~nan]), what
    assert (np.abs(g[band] - r[band]) <= 1).all(), what


def _layouts(pad):
    """(pad columns, in_off, out_off): the base on the 16-byte grid and off it."""
    return ((pad, 0, 0), (pad, 1, 1))


@gpu
@pytest.mark.parametrize("rows,in_len,fact,pad", [(1, 1, 1, 0), (3, 12, 3, 5), (2, 4096, 4096, 3), (2, 2100, 7, 1),
                                                  (1, 2 * BIG, 2, 0)])
def test_down_sample(rows, in_len, fact, pad, hip_lib):
    nout = in_len // fact
    lo = np.arange(nout, dtype=np.int64) * fact
    for name, k, s in _sample_sets(rows, in_len, 1000 + in_len % 997 + fact):
        x = np.ldexp(k.astype(np.float64), -s).astype(np.float32)
        assert np.array_equal(np.ldexp(x.astype(np.float64), s), k)
        ref, band = mean_reference(k, s, lo, lo + fact)
        for pad_, in_off, out_off in _layouts(pad):
            src = kh.GuardedInput(x, in_len + pad_, in_off=in_off, guard=IN_GUARD)
            out = kh.GuardedOutput(rows, nout, out_off=out_off)
            assert hip_lib.pss_down_sample(src.ptr, out.ptr, rows, in_len, in_len + pad_, fact, _stream()) == 0
            _check_means(out.read(), ref, band, "down_sample %s %d/%d off %d" % (name, in_len, fact, in_off))
            if fact & (fact - 1) == 0:
                assert not band.any()


def _rebin_windows(N, newlen):
    from psrsigsim_amd.utils.utils import rebin_edges
    if newlen == "hand":
        # an empty window (NaN), the whole row, single samples at both ends, overlapping windows
        return np.array([0, 5, 5, 0, N - 1, 0], dtype=np.int64), np.array([4, 5, 9, N, N, 1], dtype=np.int64)
    lo, hi = rebin_edges(N, newlen)
    assert lo.shape == (newlen,) and (0 <= lo).all() and (lo <= hi).all() and hi.max() == N
    return lo, hi


@gpu
@pytest.mark.parametrize("N,newlen", [(1000, 7), (1000, 333), (1000, 999), (1000, 1000), (1000, "hand"),
                                      (4098, 1025), ((1 << 21) + 2, BIG)])
def test_rebin(N, newlen, hip_lib):
    lo, hi = _rebin_windows(N, newlen)
    nwin = lo.size
    rows = 1 if N > 1 << 20 else 3
    dlo, dhi = _dev(lo), _dev(hi)
    for name, k, s in _sample_sets(rows, N, 2000 + N % 997 + nwin):
        x = np.ldexp(k.astype(np.float64), -s).astype(np.float32)
        ref, band = mean_reference(k, s, lo, hi)
        if newlen == "hand":
            assert np.isnan(ref[:, 1]).all() and np.isnan(ref).sum() == rows
        for pad, in_off, out_off in _layouts(6):
            src = kh.GuardedInput(x, N + pad, in_off=in_off, guard=IN_GUARD)
            out = kh.GuardedOutput(rows, nwin, out_off=out_off)
            assert hip_lib.pss_rebin(src.ptr, out.ptr, rows, N, N + pad, nwin, dlo.data_ptr(), dhi.data_ptr(),
                                     _stream()) == 0
            _check_means(out.read(), ref, band, "rebin %s %d->%s off %d" % (name, N, newlen, in_off))


# ---------------------------------------------------------------------------
# pss_clip_cast
# ---------------------------------------------------------------------------
COUNTS = (1, 255, 257, BIG)
BYTE_GUARD = 0xA5
# the reference's clip (> clip -> clip) then np.array(..., dtype=int8): truncation toward zero of the clamped value
I8_TABLE = {127.0: [(-129.7, -128), (-128.0, -128), (-0.9, 0), (0.9, 0), (126.999, 126), (127.9, 127),
                    (np.inf, 127), (-np.inf, -128)],
            100.0: [(100.5, 100), (101.0, 100)]}


def _clip_values(count, clip, seed, special):
    v = np.random.default_rng(seed).uniform(-200.0, 200.0, count).astype(np.float32)
    sp = np.asarray(special, dtype=np.float32)[:count]
    at = np.linspace(0, count - 1, sp.size).astype(np.int64) if count >= 2 * sp.size else np.arange(sp.size)
    v[at] = sp                                               # spread over the row (its last sample included)
    return v


@gpu
@pytest.mark.parametrize("count", COUNTS)
def test_clip_cast_f32(count, hip_lib):
    """min(v, clip) exactly; NaN stays NaN, -inf stays -inf, -0.0 keeps its sign."""
    from psrsigsim_amd import _lib
    clip = 100.0
    v = _clip_values(count, clip, 30 + count, [np.nan, -np.inf, np.inf, -0.0, 100.0, 100.00001, 99.99999, 3e38, -3e38])
    want = np.where(v > np.float32(clip), np.float32(clip), v)
    if count > 1:
        assert np.isnan(want).sum() == 1 and (want == -np.inf).sum() == 1 and want[np.isfinite(want)].max() == clip
    for in_off, out_off in ((0, 0), (1, 1)):
        src = kh.GuardedInput(v[None, :], count + 3, in_off=in_off, guard=IN_GUARD)
        out = kh.GuardedOutput(1, count, out_off=out_off)
        assert hip_lib.pss_clip_cast(src.ptr, out.ptr, count, clip, _lib.OUT_F32, _stream()) == 0
        assert kh.same_bits(out.read()[0], want)


def _clip_cast_i8(hip_lib, v, clip, off, in_off=0):
    """The int8 output of pss_clip_cast at byte offset ``off`` of a byte
    tensor that holds 0xA5 elsewhere; asserts the guards."""
    import torch
    from psrsigsim_amd import _lib
    G = 64
    buf = torch.full((G + off + v.size + G,), BYTE_GUARD, dtype=torch.uint8, device="cuda")
    src = kh.GuardedInput(v[None, :], v.size + 3, in_off=in_off, guard=IN_GUARD)
    assert hip_lib.pss_clip_cast(src.ptr, buf.data_ptr() + G + off, v.size, clip, _lib.OUT_I8, _stream()) == 0
    h = buf.cpu().numpy()
    assert (h[:G + off] == BYTE_GUARD).all(), "written before the output"
    assert (h[G + off + v.size:] == BYTE_GUARD).all(), "written behind the output"
    return h[G + off:G + off + v.size].view(np.int8).copy()


@gpu
@pytest.mark.parametrize("clip", sorted(I8_TABLE))
@pytest.mark.parametrize("count", COUNTS)
def test_clip_cast_i8(count, clip, hip_lib):
    vals, codes = zip(*I8_TABLE[clip])
    v = _clip_values(count, clip, 40 + count, vals)
    want = np.trunc(np.clip(np.minimum(v.astype(np.float64), clip), -128.0, 127.0)).astype(np.int8)
    # the table's values are where they were put, with the codes written down above
    sp = np.asarray(vals, dtype=np.float32)
    for x, c in zip(sp[:count], codes):
        assert (want[v == x] == c).all(), (x, c)
    for off in range(4):
        got = _clip_cast_i8(hip_lib, v, clip, off, in_off=off % 2)
        assert np.array_equal(got, want), (count, clip, off)


def _finalize_i8(hip_lib, v, clip):
    """k_out_finalize's int8 cast of the window means of one loaded row
    ``v``: a run with no stage but observe()'s down-sampled copy (windows of
    one sample: the mean is the sample)."""
    import ctypes
    import torch
    from psrsigsim_amd import _lib
    n = v.size
    data = _dev(v.astype(np.float32)[None, :])
    acc = torch.zeros(n, dtype=torch.float64, device="cuda")
    out = torch.full((n,), 0x55, dtype=torch.int8, device="cuda")
    p = _lib.PssPipeline()
    p.nchan, p.nsamp, p.ld, p.data, p.src = 1, n, n, data.data_ptr(), _lib.SRC_LOAD
    p.out_kind, p.out, p.clip = _lib.OUT_I8, out.data_ptr(), clip
    p.out_len, p.out_step, p.out_acc = n, 1.0, acc.data_ptr()
    _lib.check(hip_lib.pss_run(ctypes.byref(p), _stream()), "pss_run")
    return out.cpu().numpy()


@gpu
def test_clip_cast_i8_nan_is_pinned(hip_lib):
    """A PIN of what the kernels do, not a parity claim: the reference's
    np.array(nan, dtype=int8) is undefined.  k_clip_cast clamps with
    fmaxf(NaN, -128) = -128 (fmaxf returns its other argument), and
    k_out_finalize (observe()'s resampled int8 copy) gives the same value on
    the same input."""
    v = np.array([np.nan, 3.7, -np.nan, -200.0, 200.0, np.nan, 0.0, -0.5], dtype=np.float32)
    want = np.array([-128, 3, -128, -128, 127, -128, 0, 0], dtype=np.int8)
    for off in range(4):
        assert np.array_equal(_clip_cast_i8(hip_lib, v, 127.0, off), want), off
    assert np.array_equal(_finalize_i8(hip_lib, v, 127.0), want)


# ---------------------------------------------------------------------------
# folds
# ---------------------------------------------------------------------------
def _ints(shape, seed):
    return np.random.default_rng(seed).integers(0, 1 << 20, shape).astype(np.float32)


@gpu
@pytest.mark.parametrize("nchan,npbins,n_fold,pad", [(3, 64, 3, 5), (2, 65, 4, 0), (1, 2, 1, 3), (2, 64, 0, 0),
                                                     (1, 2 * BIG, 1, 2)])
def test_fold(nchan, npbins, n_fold, pad, hip_lib):
    half = npbins // 2
    n = npbins + n_fold * half
    x = _ints((nchan, n), 50 + npbins % 997 + n_fold)
    want = x[:, npbins:].astype(np.float64).reshape(nchan, n_fold, half).sum(axis=1).astype(np.float32)
    if n_fold == 0:
        assert not want.any()
    for pad_, in_off, out_off in _layouts(pad):
        src = kh.GuardedInput(x, n + pad_, in_off=in_off, guard=IN_GUARD)
        out = kh.GuardedOutput(nchan, half, out_off=out_off)
        assert hip_lib.pss_fold(src.ptr, out.ptr, nchan, n + pad_, npbins, n_fold, _stream()) == 0
        assert kh.same_bits(out.read(), want), (in_off, out_off)


@gpu
@pytest.mark.parametrize("nper,nbin", [(p, b) for p in (1, 7, 8, 9, 17) for b in (1, 5, 244)] + [(1, BIG)])
def test_fold_periods(nper, nbin, hip_lib):
    """The trailing samples of an incomplete period hold the guard and are not read."""
    nchan = 1 if nbin == BIG else 2
    n = nper * nbin
    pad = min(max(1, nbin - 1), 7)
    x = _ints((nchan, n), 60 + nper + nbin % 997)
    want = x.astype(np.float64).reshape(nchan, nper, nbin).sum(axis=1).astype(np.float32)
    for in_off, out_off in ((0, 0), (1, 1)):
        src = kh.GuardedInput(x, n + pad, in_off=in_off, guard=IN_GUARD)
        out = kh.GuardedOutput(nchan, nbin, out_off=out_off)
        assert hip_lib.pss_fold_periods(src.ptr, out.ptr, nchan, n + pad, nbin, nper, _stream()) == 0
        assert kh.same_bits(out.read(), want), (in_off, out_off)


# ---------------------------------------------------------------------------
# pss_null_shift
# ---------------------------------------------------------------------------
def _null_rows(count):
    """(name, row, status): status 0 a unique maximum, 1 a tie, 2 a NaN."""
    base = np.random.default_rng(70 + count).random(count).astype(np.float32)

    def peak(*at, value=2.0):
        r = base.copy()
        r[list(at)] = value
        return r

    yield "maximum at 0", peak(0), 0
    yield "maximum at count - 1", peak(count - 1), 0
    for i in (255, 256):                                     # the boundary between the threads' strides
        if i < count:
            yield "maximum at %d" % i, peak(i), 0
    yield "a unique +inf", peak(count // 2, value=np.inf), 0
    yield "NaN only", np.full(count, np.nan, np.float32), 2
    if count == 1:
        yield "one -inf", np.full(1, -np.inf, np.float32), 0
        return
    if count > 256:
        yield "tie at i, i + 256 (one thread)", peak(count - 257, count - 1), 1
    yield "tie at i, i + 1 (two threads)", peak(count - 2, count - 1), 1
    yield "all equal", np.full(count, 0.5, np.float32), 1
    yield "all -inf", np.full(count, -np.inf, np.float32), 1
    r = peak(count - 1)
    r[0] = np.nan
    yield "NaN before the maximum", r, 2
    r = peak(0)
    r[count - 1] = np.nan
    yield "NaN after the maximum", r, 2


@gpu
@pytest.mark.parametrize("count", [1, 2, 255, 256, 257, 5000])
def test_null_shift(count, hip_lib):
    """out = [count // 2 - argmax(row[:count]), status]; the words past
    ``count`` hold 2^20, above every maximum, and are not seen."""
    seen = set()
    for name, row, status in _null_rows(count):
        for in_off in (0, 1):
            src = kh.GuardedInput(row[None, :], count + 5, in_off=in_off, guard=IN_GUARD)
            out = kh.GuardedOutput(1, 2, out_off=in_off, guard=-77, dtype=np.int64)
            assert hip_lib.pss_null_shift(src.ptr, count, out.ptr, _stream()) == 0
            got = out.read()[0]
            assert got[1] == status, (name, count, got)
            if status == 0:
                assert got[0] == count // 2 - int(np.argmax(row)), (name, count, got)
        seen.add(status)
    assert seen == {0, 1, 2} or count == 1
