"""The stream definition (tests/philox_ref.py) on the CPU: known answers of
the round function, and the statistical properties the definition promises --
marginals, tails and the absence of correlation along every axis of the key
(sample, pair member, channel, purpose, call, either half of the seed) -- at
2^20 draws per stream, a size no GPU test should use.  The device is held
against the same definition draw by draw in tests/test_gpu_draw_streams.py.

Seeds are fixed, so every check is deterministic.  They were not searched
for: the first seeds tried (SEED, and SEED with another high word) pass all
checks below; the smallest KS p-value is 0.069 (chi2(1)) and the largest
correlation 3.4 / sqrt(n) (chi2(1); at most 2.0 / sqrt(n) for the others;
per-df figures in profiles/draw_streams/README.md)."""
import numpy as np
import pytest
from scipy import stats

from tests import philox_ref as R

N = 1 << 20
SEED = 0x9E3779B97F4A7C15
SEED_HI = SEED ^ (0x5A5A5A5A << 32)        # the same low word, another high word
CALL = 7
DFS = (0.5, 1.0, 1.5, 2.0, 3.7, 100.0, 11190.0)


def _u(word):
    """The float32 uniform of a word, by scalar arithmetic."""
    return float(np.float32(word) * np.float32(2.0 ** -32) + np.float32(2.0 ** -33))


def _words(s):
    return [int(w, 16) for w in s.split()]


# (counter, key, 10 rounds: Random123 kat_vectors philox4x32; 7 rounds: regression values of this model)
KAT = [("00000000 00000000 00000000 00000000", "00000000 00000000",
        "6627e8d5 e169c58d bc57ac4c 9b00dbd8", "5f6fb709 0d893f64 4f121f81 4f730a48"),
       ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff",
        "408f276d 41c83b0e a20bc7c6 6d5451fd", "5207ddc2 45165e59 4d8ee751 8c52f662"),
       ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0",
        "d16cfe09 94fdcceb 5001e420 24126ea1", "4dfccaba 190a87f0 c47362ba b6b5242a")]


@pytest.mark.parametrize("ctr,key,r10,r7", KAT)
def test_philox_known_answers(ctr, key, r10, r7):
    for rounds, want in ((10, r10), (7, r7)):
        got = R.philox(*_words(ctr), *_words(key), rounds=rounds)
        assert [int(w) for w in got] == _words(want), rounds
    # the default is the device's round count, and arrays give what scalars give
    c = [np.array([w, w]) for w in _words(ctr)]
    got = R.philox(*c, *_words(key))
    assert [int(w[1]) for w in got] == _words(r7)


def test_keying_layout():
    """bits() puts (a, tag, b, call << 4 | purpose) in the counter and the two
    halves of the seed in the key; chi2_rows / normal_rows take block n >> 2
    (pairs: n >> 1) of global row b, and a ragged tail is a prefix."""
    got = R.bits(3, 9, 5, SEED, 0x0FFFFFFF, 4)
    want = R.philox(3, 9, 5, (0x0FFFFFFF << 4 | 4) & 0xFFFFFFFF, SEED & 0xFFFFFFFF, SEED >> 32)
    assert [int(w) for w in got] == [int(w) for w in want]
    for df in (1.0, 3.7, 0.5):
        full = R.chi2_rows(8, 0, 4099, df, SEED, CALL, 5)[0]
        np.testing.assert_array_equal(R.chi2_rows(3, 5, 1001, df, SEED, CALL, 5)[0], full[5:8, :1001])
    full = R.normal_rows(8, 0, 4099, SEED, CALL, 4)[0]
    np.testing.assert_array_equal(R.normal_rows(3, 5, 1001, SEED, CALL, 4)[0], full[5:8, :1001])
    # chi2(1) from first principles, one draw: block 1, element 2 (n = 6)
    r = R.philox(1, 0, 2, CALL << 4 | 5, SEED & 0xFFFFFFFF, SEED >> 32)
    u = _u(int(r[2]))
    v = (((int(r[3]) << 1) & 0xFFFFFFFF) >> 9) / 2.0 ** 23
    x, _, _, h = R.chi2_rows(1, 2, 8, 1.0, SEED, CALL, 5)
    assert abs(x[0, 6] - (-np.log(u)) * (1 + np.cos(2 * np.pi * v))) < 1e-12
    assert h[0, 6] == -np.log(u)


def test_pair_sampler_bookkeeping():
    """Retry depth, margin and the 1 + c z <= 0 count of the pair sampler
    against a scalar restatement of one row."""
    df, n, chan = 0.5, 2000, 3
    st = {}
    x, depth, margin, h = R.chi2_rows(1, chan, n, df, SEED, CALL, 5, stats=st)
    assert h is None and depth.max() >= 2 and st["neg_rejects"] >= 1
    shape, boost, d, c = R.mt_params(df)
    assert boost and shape == 0.25
    negs = 0
    for i in range(n):
        m, hh = i >> 1, i & 1
        mg = np.inf
        for t in range(64):
            tag = 1 if t == 0 else ((hh + 1) << 16) | t
            r = [int(w) for w in R.bits(m, tag, chan, SEED, CALL, 5)]
            l = np.sqrt(-2 * np.log(_u(r[0])))
            ang = 2 * np.pi * (r[1] >> 9) / 2.0 ** 23
            z = l * (np.sin(ang) if (t == 0 and hh) else np.cos(ang))
            u = _u(r[3] if (t == 0 and hh) else r[2])
            w = 1 + c * z
            mg = min(mg, abs(w) / c)
            if w <= 0:
                negs += 1
                continue
            v = w ** 3
            gap = z * z / 2 + d * (1 - v + np.log(v)) - np.log(u)
            mg = min(mg, abs(gap))
            if gap > 0:
                break
        ub = [int(w) for w in R.bits(m, 0xFFFF0000, chan, SEED, CALL, 5)]
        want = 2 * d * v * _u(ub[hh]) ** (1 / shape)
        assert depth[0, i] == t and abs(x[0, i] - want) <= 1e-12 * want and abs(margin[0, i] - mg) <= 1e-12, i
    assert negs == st["neg_rejects"]


# ---------------------------------------------------------------------------
# properties of the definition
# ---------------------------------------------------------------------------
def _corr(a, b):
    a = a - a.mean()
    b = b - b.mean()
    return float(np.dot(a, b) / np.sqrt(np.dot(a, a) * np.dot(b, b)))


def _streams(draw):
    """The streams whose pairwise independence is checked: draw(chan, seed,
    call, purpose) -> one row of N draws."""
    base = draw(10, SEED, CALL, R.P_PULSE)
    return base, {"channel c+1": draw(11, SEED, CALL, R.P_PULSE),
                  "purpose 3": draw(10, SEED, CALL, R.P_REP),
                  "purpose 4": draw(10, SEED, CALL, R.P_NOISE),
                  "call k+1": draw(10, SEED, CALL + 1, R.P_PULSE),
                  "seed high word": draw(10, SEED_HI, CALL, R.P_PULSE)}


def _check_independence(base, others, tag):
    n = base.size
    bound = 5.0 / np.sqrt(n)
    pairs = [("lag %d" % l, base[:-l], base[l:]) for l in (1, 2, 3, 4, 8)]
    pairs.append(("pair members", base[0::2], base[1::2]))
    pairs += [(k, base, v) for k, v in others.items()]
    pairs.append(("purpose 3 vs 4", others["purpose 3"], others["purpose 4"]))
    worst = 0.0
    for name, a, b in pairs:
        for power in (1, 2):
            r = _corr(a ** power, b ** power)
            worst = max(worst, abs(r) * np.sqrt(a.size))
            assert abs(r) <= 5.0 / np.sqrt(a.size), (tag, name, "x^%d" % power, r, bound)
    return worst


def _check_marginal(x, dist, tag):
    n = x.size
    p = stats.kstest(x, dist.cdf).pvalue
    assert p > 0.01, (tag, "KS", p)
    q = 1e-4
    share = float((x > dist.ppf(1 - q)).mean())
    assert abs(share - q) <= 5 * np.sqrt(q * (1 - q) / n), (tag, "tail", share)
    return p, share


@pytest.mark.parametrize("df", DFS)
def test_chi2_definition_properties(df):
    def draw(chan, seed, call, purpose):
        return R.chi2_rows(1, chan, N, df, seed, call, purpose)[0][0]

    base, others = _streams(draw)
    p, share = _check_marginal(base, stats.chi2(df), df)
    worst = _check_independence(base, others, df)
    print("chi2(%g): KS p %.3f, tail share %.3e, largest |r| sqrt(n) %.2f" % (df, p, share, worst))


def test_normal_definition_properties():
    def draw(row, seed, call, purpose):
        return R.normal_rows(1, row, N, seed, call, purpose)[0][0]

    base, others = _streams(draw)
    p, share = _check_marginal(base, stats.norm, "normal")
    lo = float((base < stats.norm.ppf(1e-4)).mean())
    assert abs(lo - 1e-4) <= 5 * np.sqrt(1e-4 / N), lo
    worst = _check_independence(base, others, "normal")
    print("normal: KS p %.3f, tail shares %.3e / %.3e, largest |r| sqrt(n) %.2f" % (p, share, lo, worst))


def test_fill_cases_are_not_vacuous():
    """Every pss_chi2_fill case of tests/test_gpu_draw_streams.py, from the
    model alone: the undecided share is under the cap, every df != 1 case has
    a retry, every df = 0.5 case a second retry and a 1 + c z <= 0 reject."""
    cases = R.fill_cases()
    assert len(cases) == 45 and {c[0] for c in cases} == set(R.FILL_DFS)
    for df, chan0, call, purpose in cases:
        counts = R.fill_model(df, chan0, call, purpose)[4]
        R.check_fill_counts(df, counts)
        if (chan0, call, purpose) == (0, 1, R.P_TEST):
            print("df %g: %s" % (df, counts))
