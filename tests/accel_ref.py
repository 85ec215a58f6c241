"""NumPy / Python-integer restatement of the acceleration resampler (no GPU,
no package code):

* ``clamp_step``     -- K(r) and sg(r) of a table entry ``kappa`` (an integer in
  the int64 range): ``K = min(|kappa|, 2^63 // T)``;
* ``shift`` / ``index`` -- ``s(t) = (t (T - t) K + 2^63) >> 64`` with Python
  integers (the 128-bit product is exact) and ``idx(t) = clip(t + sg s(t), 0,
  T - 1)``; ``index_unclamped`` leaves the last clip out;
* ``resample``       -- ``pss_accel_resample`` (include/pss_hip.h): ``out[r][t]
  = x[i(r)][idx_r(t)] - sub[r]`` in float32, the bits copied without ``sub``;
* ``kappa_of_shift`` -- the table entry of a mid-observation shift of ``s_max``
  samples, ``round(4 |s_max| 2^64 / T^2)`` with its sign, by ``Fraction``;
* ``kappa_of_accel`` -- the table entry of ``Backend.accel_shift_step``;
* ``accel_signal``   -- the accelerated pulse train of the issue's study.
"""
from fractions import Fraction

import numpy as np

C_M_S = 299792458.0
TWO63, TWO64 = 1 << 63, 1 << 64


def clamp_step(kappa, T):
    kappa = int(kappa)
    assert -TWO63 <= kappa < TWO63
    return min(abs(kappa), TWO63 // int(T)), (-1 if kappa < 0 else 1)


def shift(T, K, t=None):
    """s(t) for t in ``t`` (default 0 .. T - 1): a list of Python ints."""
    T = int(T)
    ts = range(T) if t is None else t
    return [(int(v) * (T - int(v)) * K + TWO63) >> 64 for v in ts]


def index_unclamped(T, kappa, n_out=None):
    K, sg = clamp_step(kappa, T)
    n = int(T) if n_out is None else int(n_out)
    return np.arange(n, dtype=np.int64) + sg * np.array(shift(T, K, range(n)), dtype=np.int64)


def index(T, kappa, n_out=None):
    return np.clip(index_unclamped(T, kappa, n_out), 0, int(T) - 1)


def resample(x, src, kappa, sub=None, n_out=None):
    """out float32 [nrows][n_out]; ``x`` float32 [nser][T]."""
    x = np.asarray(x, dtype=np.float32)
    nser, T = x.shape
    n = T if n_out is None else int(n_out)
    out = np.empty((len(src), n), dtype=np.float32)
    for r, (i, k) in enumerate(zip(src, kappa)):
        row = x[min(max(int(i), 0), nser - 1)][index(T, k, n)]
        if sub is not None:
            with np.errstate(all="ignore"):
                row = row - np.float32(sub[r])
            assert row.dtype == np.float32
        out[r] = row
    return out


def _round_half_up(q):
    q = q + Fraction(1, 2)
    return q.numerator // q.denominator


def kappa_of_shift(s_max, T):
    """sign(s_max) floor(4 |s_max| 2^64 / T^2 + 1/2)."""
    k = _round_half_up(Fraction(4 * abs(int(s_max)) * TWO64, int(T) ** 2))
    return k if s_max >= 0 else -k


def alpha_of_accel(accel, samprate_MHz):
    """alpha = -a / (2 c fs) per sample as an exact Fraction of the float64
    inputs (fs = the float64 product samprate * 1e6)."""
    return -Fraction(float(accel)) / (2 * Fraction(C_M_S) * Fraction(float(samprate_MHz) * 1e6))


def kappa_of_accel(accel, samprate_MHz):
    al = alpha_of_accel(accel, samprate_MHz)
    k = _round_half_up(abs(al) * TWO64)
    return k if al >= 0 else -k


def accel_signal(T=65536, period=128.37, s_max=96, amp=0.6, width=0.02, seed=0):
    """x = N(0, 1) + amp exp(-(d / width)^2 / 2), d the distance of
    frac((t - alpha t (T - t)) / period) to the nearest integer, alpha =
    4 s_max / T^2: a pulse train that the resampling of shift +s_max
    straightens.  float32 [T]."""
    rng = np.random.default_rng(seed)
    t = np.arange(T, dtype=np.float64)
    alpha = 4.0 * s_max / float(T) ** 2
    ph = (t - alpha * t * (T - t)) / period
    d = ph - np.round(ph)
    return (rng.standard_normal(T) + amp * np.exp(-0.5 * (d / width) ** 2)).astype(np.float32)
