#!/usr/bin/env python
"""Statistics study of the device's chi2(1) draws on the CPU.

The stream definition itself -- Philox4x32-7, the keying, the chi2(1), the
Marsaglia-Tsang pair and the Box-Muller normal samplers -- is
tests/philox_ref.py (float64, held against the device draw for draw by
tests/test_gpu_draw_streams.py); `philox` is imported from there.  `chi2_1`
below is the study's own variant of the chi2(1) sampler: the "cos2" form
h (1 +- cos 4 pi v), h = -ln u, of pss::chi2_1x4 with the fp32 roundings of
its last three operations, or the earlier "two-trig" form, at any number of
rounds; every draw n of a row takes element n & 3 of block n >> 2 (counter
(n >> 2, 0, channel, call << 4 | purpose), key = seed).

Agreement with the device (measured, profiles/draw_streams/README.md): not
bit for bit -- the device's logarithm and cosine are the hardware's
approximations.  Over 45 fills of 12297 draws a device chi2(1) draw is within
3.9e-7 h of tests/philox_ref.py's (h = -ln u the scale of its pair), given
that model's float32 uniform; `chi2_1` below keeps the uniform in float64,
which moves h by up to 2^-25 / u (up to 8e-3 of a small h) and a draw by less
than 6e-8 absolute.  Either is far below what a statistic of 10^5 .. 10^8
draws resolves, so the quality of the generator can be studied here at sample
sizes no GPU test would use:

  tools/philox_model.py study     -> profiles/r03/philox_quality.txt

compares R = 7 (both Box-Muller forms) and R = 10 on (a) KS p-values of the on-pulse selection of
tests/test_gpu_stats.py::test_search_pulse_draws_are_chi2_1 over 400 seeds
(their distribution must be uniform), (b) lag correlations over 6.7e7
draws, (c) mean / second moment over 6.7e7 draws."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.philox_ref import MASK, philox  # noqa: E402


def chi2_1(n, chan, seed, call, purpose, rounds=7, form="cos2"):
    """Draws n = 0 .. n-1 of global channel `chan`.  form "cos2" (the device's
    sampler): h (1 +- cos 4 pi v), h = -ln u, with the
    fp32 roundings of the device's last three operations (so the cancellation
    of the small member of a pair is modelled); "two-trig": the previous
    -2 ln u cos^2 / sin^2 form, float64."""
    blocks = np.arange((n + 3) // 4, dtype=np.uint64)
    r = philox(blocks, 0, chan, (call << 4) | purpose, seed & 0xFFFFFFFF, seed >> 32, rounds)
    u01 = lambda x: x.astype(np.float64) * 2.0 ** -32 + 2.0 ** -33
    fr = lambda x: (x >> np.uint64(9)).astype(np.float64) * 2.0 ** -23
    if form == "cos2":
        f32 = np.float32
        fr2 = lambda x: ((x << np.uint64(1)) & MASK).astype(np.uint64)
        h0, h1 = f32(-np.log(u01(r[0]))), f32(-np.log(u01(r[2])))
        c0, c1 = f32(np.cos(2 * np.pi * fr(fr2(r[1])))), f32(np.cos(2 * np.pi * fr(fr2(r[3]))))
        # fused h (1 +- c): the product exact in float64, one fp32 rounding
        d0, d1 = h0.astype(np.float64) * c0, h1.astype(np.float64) * c1
        out = np.stack([f32(h0 + d0), f32(h0 - d0), f32(h1 + d1), f32(h1 - d1)], 1).astype(np.float64)
        return out.ravel()[:n]
    l0, l1 = -2 * np.log(u01(r[0])), -2 * np.log(u01(r[2]))
    v0, v1 = 2 * np.pi * fr(r[1]), 2 * np.pi * fr(r[3])
    out = np.stack([l0 * np.cos(v0) ** 2, l0 * np.sin(v0) ** 2, l1 * np.cos(v1) ** 2, l1 * np.sin(v1) ** 2], 1)
    return out.ravel()[:n]


def study(out):
    from scipy import stats
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar, GaussProfile
    sig = FilterBankSignal(1400, 400, Nsubband=2, fold=False)
    psr = Pulsar(0.005, 1.0, profiles=GaussProfile(0.5, 0.1, 1))
    psr.make_pulses(sig, tobs=(1 << 18) * 20.48e-6)
    n = sig._ncols
    spp = (sig._samprate_MHz() * 0.005) * 1e6
    sel = psr.Profiles.calc_profiles((np.arange(n) / spp) % 1)[0] > 0.5
    lines = []
    for R, form in ((7, "cos2"), (7, "two-trig"), (10, "two-trig")):
        ps = np.array([stats.kstest(chi2_1(n, 0, s, 1, 1, R, form)[sel], stats.chi2(1).cdf).pvalue
                       for s in range(1, 401)])
        lag = {}
        m1 = m2 = 0.0
        small = 0
        for ch in range(8):
            x = chi2_1(1 << 23, 10 + ch, 4242, 1, 1, R, form)
            small += int((x < 1e-4).sum())
            m1 += x.mean() / 8
            m2 += (x * x).mean() / 8
            x = x - 1.0
            for l in (1, 2, 3, 4, 5, 8):
                lag[l] = lag.get(l, 0.0) + np.mean(x[:-l] * x[l:]) / 2.0 / 8
        se = 1.0 / np.sqrt(8 * (1 << 23))
        lines.append("Philox4x32-%d, %s sampler: on-pulse KS over 400 seeds: frac p<0.01 %.4f, p<0.05 %.4f, "
                     "uniformity of the p-values (KS) %.3f; P(x < 1e-4) = %.3e (chi2(1): %.3e)"
                     % (R, form, (ps < .01).mean(), (ps < .05).mean(), stats.kstest(ps, "uniform").pvalue,
                        small / (8.0 * (1 << 23)), stats.chi2(1).cdf(1e-4)))
        lines.append("  6.7e7 draws: mean-1 %.2e (SE %.1e), E[x^2]/3-1 %.2e (SE %.1e); lag correlations in SE units %s"
                     % (m1 - 1, np.sqrt(2 / 6.7e7), m2 / 3 - 1, np.sqrt(96 / 6.7e7) / 3,
                        {l: round(v / se, 2) for l, v in lag.items()}))
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "study":
        study(sys.argv[2] if len(sys.argv) > 2 else "profiles/r03/philox_quality.txt")
