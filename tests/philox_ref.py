"""The random streams, restated in NumPy float64 ("The
random streams"): the executable definition that the device's draws are held
against, draw by draw (tests/test_gpu_draw_streams.py), and whose statistical
properties are examined on the CPU (tests/test_philox_model.py).

It restates psrsigsim_amd/csrc/pss_device.hpp (philox, Rng, chi2_1x4,
normal_x4, mt_try / mt_retry / chi2_pair) and draw4 of pss_stages.hpp from
their definitions -- every logarithm, cosine and power in float64, none of
the fp32 forms (the fused h (1 +- c), log1p_minus, the squeeze); the one
float32 quantity is the uniform itself, which the stream defines on the
float32 grid -- so an
agreement with the device is an agreement with the definition, not with a
copy of the code.

Keying.  A Philox4x32-7 block has counter (a, tag, b, call << 4 | purpose) and
key (seed & 0xFFFFFFFF, seed >> 32).  Purposes: 1 pulses, 2 null boxes,
3 null replacements, 4 noise, 5 tests.  For the draws of a row, b is the
GLOBAL channel (the row index for pss_normal_add) and

  chi2(1), normals   a = n >> 2 (low 32 bits), tag = n >> 34: one block per
                     four consecutive samples
  chi2(df != 1)      a = n >> 1, the pair index; tag 1 holds attempt 0 of both
                     members, tag (h + 1) << 16 | t retry t = 1 .. 63 of
                     member h, tag 0xFFFF0000 the boost uniforms (df < 2)

Uniforms: u = (x + 1/2) 2^-32 rounded to float32, in (0, 1] (u01 below: the
float32 grid is part of the definition); angles: the top 23 bits of a word,
v = (x >> 9) 2^-23 turns.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
ROUNDS = 7                      # kPhiloxRounds
P_PULSE, P_BOX, P_REP, P_NOISE, P_TEST = 1, 2, 3, 4, 5
TAG_FIRST, TAG_BOOST, MAX_TRIES = 1, 0xFFFF0000, 64


def philox(c0, c1, c2, c3, k0, k1, rounds=ROUNDS):
    """Philox4x32-`rounds` (Salmon et al. 2011) of counters (c0, c1, c2, c3)
    (arrays or scalars, broadcast) under key (k0, k1): four uint64 arrays
    holding the 32-bit output words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) & MASK for x in (c0, c1, c2, c3)])
    k0, k1 = np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)
    for _ in range(rounds):
        p0, p1 = c0 * M0, c2 * M1                      # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = ((p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK)
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def bits(a, tag, b, seed, call, purpose, rounds=ROUNDS):
    """The block of stream position (a, b) and attempt `tag` (Rng::bits)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    word = ((int(call) << 4) | int(purpose)) & 0xFFFFFFFF
    return philox(a, tag, b, word, seed & 0xFFFFFFFF, seed >> 32, rounds)


def u01(x):
    """The uniform of a word: (x + 1/2) 2^-32 AS A FLOAT32, float(x) 2^-32 +
    2^-33 with float(x) the word rounded to 24 bits and the sum rounded once
    (pss::u01).  The rounding is part of the definition, not an error of the
    device: the uniform lives on the float32 grid -- all 32 bits of the word
    below 2^-8, steps of 2^-24 above 1/2, exactly 1 for the top 128 words, so
    it lies in (0, 1] and -ln u is 0 with probability 2^-25.  Against the
    unrounded value -ln u moves by up to 2^-25 / u, which near u = 1 is far
    more than any rounding of the logarithm (measured on the device: up to
    8e-3 of h over 12297 draws); every transcendental below is float64 OF THIS
    float32 uniform."""
    x = np.asarray(x, dtype=np.uint64).astype(np.float32)
    return (x * np.float32(2.0 ** -32) + np.float32(2.0 ** -33)).astype(np.float64)


def frac23(x):
    """[0, 1) on a 23-bit grid: the top 23 bits of the word."""
    return ((x & MASK) >> np.uint64(9)).astype(np.float64) * 2.0 ** -23


def _rowgrid(nrows, b0, count):
    """Stream positions a = 0 .. count - 1 of rows b0 .. b0 + nrows - 1, as
    [nrows, count] arrays (a's high half is the tag of the 4-sample blocks)."""
    a = np.arange(count, dtype=np.uint64)[None, :]
    b = (np.uint64(b0) + np.arange(nrows, dtype=np.uint64))[:, None]
    return np.broadcast_arrays(a, b)


def _chi2_1(nrows, chan0, n, seed, call, purpose, rounds):
    a, b = _rowgrid(nrows, chan0, (n + 3) // 4)
    r = bits(a & MASK, a >> S32, b, seed, call, purpose, rounds)
    h0, h1 = -np.log(u01(r[0])), -np.log(u01(r[2]))
    # h (1 +- cos 4 pi v), 4 pi v mod 2 pi from the top 23 bits of word << 1;
    # as 2 h cos^2 / 2 h sin^2 of the half angle, which does not cancel
    t0 = np.pi * frac23(r[1] << np.uint64(1))
    t1 = np.pi * frac23(r[3] << np.uint64(1))
    x = np.stack([2 * h0 * np.cos(t0) ** 2, 2 * h0 * np.sin(t0) ** 2,
                  2 * h1 * np.cos(t1) ** 2, 2 * h1 * np.sin(t1) ** 2], axis=2).reshape(nrows, -1)[:, :n]
    h = np.stack([h0, h0, h1, h1], axis=2).reshape(nrows, -1)[:, :n]
    return x, np.zeros(x.shape, dtype=np.int64), np.full(x.shape, np.inf), h


def mt_params(df):
    """Marsaglia-Tsang (2000) constants of Gamma(shape = df / 2): shape < 1
    is drawn as Gamma(shape + 1) U^(1 / shape)."""
    shape = 0.5 * float(df)
    boost = shape < 1.0
    d = (shape + 1.0 if boost else shape) - 1.0 / 3.0
    return shape, boost, d, 1.0 / np.sqrt(9.0 * d)


def _mt_try(z, u, d, c):
    """One attempt: (accepted, v, margin, rejected by 1 + c z <= 0)."""
    w = 1.0 + c * z
    neg = w <= 0.0
    v = np.where(neg, 1.0, w) ** 3
    gap = 0.5 * z * z + d * (1.0 - v + np.log(v)) - np.log(u)
    margin = np.minimum(np.where(neg, np.inf, np.abs(gap)), np.abs(w) / c)
    return (~neg) & (gap > 0.0), v, margin, neg


def _normal_pair(rx, ry):
    l = np.sqrt(-2.0 * np.log(u01(rx)))
    t = 2.0 * np.pi * frac23(ry)
    return l * np.cos(t), l * np.sin(t), l


def _chi2_pairs(nrows, chan0, n, df, seed, call, purpose, rounds, stats):
    shape, boost, d, c = mt_params(df)
    m, b = _rowgrid(nrows, chan0, (n + 1) // 2)
    r = bits(m, TAG_FIRST, b, seed, call, purpose, rounds)
    z0, z1, _ = _normal_pair(r[0], r[1])
    ub = bits(m, TAG_BOOST, b, seed, call, purpose, rounds) if boost else None
    out, depth, margin = [], [], []
    neg_rejects = 0
    for h, (z, u) in enumerate(((z0, u01(r[2])), (z1, u01(r[3])))):
        ok, v, mg, neg = _mt_try(z, u, d, c)
        neg_rejects += int(neg.sum())
        dep = np.zeros(m.shape, dtype=np.int64)
        todo = np.nonzero(~ok)
        for t in range(1, MAX_TRIES):
            if todo[0].size == 0:
                break
            rt = bits(m[todo], ((h + 1) << 16) | t, b[todo], seed, call, purpose, rounds)
            zt = _normal_pair(rt[0], rt[1])[0]
            okt, vt, mgt, negt = _mt_try(zt, u01(rt[2]), d, c)
            neg_rejects += int(negt.sum())
            dep[todo] = t
            mg[todo] = np.minimum(mg[todo], mgt)
            v[todo] = np.where(okt, vt, 1.0)          # (63 rejections in a row leave d itself)
            todo = tuple(i[~okt] for i in todo)
        x = 2.0 * d * v
        if boost:
            x = x * u01(ub[h]) ** (1.0 / shape)
        out.append(x)
        depth.append(dep)
        margin.append(mg)
    if stats is not None:
        stats["neg_rejects"] = stats.get("neg_rejects", 0) + neg_rejects
    pack = lambda p: np.stack(p, axis=2).reshape(nrows, -1)[:, :n]
    return pack(out), pack(depth), pack(margin), None


def chi2_rows(nrows, chan0, n, df, seed, call, purpose, rounds=ROUNDS, stats=None):
    """Draws 0 .. n-1 of global channels chan0 .. chan0 + nrows - 1 (draw4 of
    pss_stages.hpp, pss_chi2_fill): (x, depth, margin, h), [nrows, n] each.

    df == 1: h (1 + cos 4 pi v), h (1 - cos 4 pi v) per (u, v) word pair of
    the block, h = -ln u; `h` is the pair scale of every draw, depth 0, margin
    inf.  Otherwise the Marsaglia-Tsang pair sampler: x = 2 d v [U^(1/shape)],
    `depth` the number of retries the draw took, `margin` the smallest, over
    the attempts it made, of |z^2/2 + d (1 - v + ln v) - ln u| and
    |1 + c z| / c -- how far the nearest accept / reject decision was from
    going the other way (an fp32 evaluation may settle a decision closer than
    its own error differently; the draw then comes from another block) --
    and h is None.  `stats` (a dict) collects "neg_rejects", the number of
    attempts rejected by 1 + c z <= 0."""
    if float(df) == 1.0:
        return _chi2_1(nrows, chan0, n, seed, call, purpose, rounds)
    return _chi2_pairs(nrows, chan0, n, df, seed, call, purpose, rounds, stats)


def normal_rows(nrows, row0, n, seed, call, purpose, rounds=ROUNDS):
    """N(0, 1) draws 0 .. n-1 of rows row0 .. (normal_x4: the amplitude
    pulses, purpose 1 keyed by global channel; pss_normal_add, purpose 4 keyed
    by row): the four Box-Muller normals l0 (cos, sin) 2 pi v0, l1 (cos, sin)
    2 pi v1 of block n >> 2.  Returns (z, l), l = sqrt(-2 ln u) of each draw."""
    a, b = _rowgrid(nrows, row0, (n + 3) // 4)
    r = bits(a & MASK, a >> S32, b, seed, call, purpose, rounds)
    c0, s0, l0 = _normal_pair(r[0], r[1])
    c1, s1, l1 = _normal_pair(r[2], r[3])
    pack = lambda p: np.stack(p, axis=2).reshape(nrows, -1)[:, :n]
    return pack([c0, s0, c1, s1]), pack([l0, l0, l1, l1])


# ---------------------------------------------------------------------------
# The pss_chi2_fill cases of tests/test_gpu_draw_streams.py (here, so that
# tests/test_philox_model.py can check without a GPU that none goes vacuous).
# ---------------------------------------------------------------------------
FILL_SEED = 0x9E3779B97F4A7C15          # (a non-zero high word)
FILL_ROWS, FILL_N = 3, 4099             # a ragged tail of 3 (df = 1), of 1 (pairs)
FILL_DFS = (1.0, 0.5, 1.5, 2.0, 3.7, 100.0, 11190.0)
EPS = 1e-3                              # a draw whose margin is below this is undecided
UNDECIDED_CAP = 5e-3                    # the share of them a case may hold


def fill_cases():
    """(df, chan0, call, purpose): every df at one keying, every keying at
    df = 1 and df = 0.5.  The one keying is (0, 1, P_TEST): at df = 11190 the
    sampler retries 4.9e-6 of its draws (measured over 2^24 of the model's), so
    of the twenty keyings only this one and (5, 0x0FFFFFFF, P_BOX) hold a
    retry among their 12297 draws (two and one)."""
    cases = [(df, 0, 1, P_TEST) for df in FILL_DFS]
    for df in (1.0, 0.5):
        for chan0 in (0, 5):
            for call in (1, 0x0FFFFFFF):
                for purpose in (1, 2, 3, 4, 5):
                    if (df, chan0, call, purpose) not in cases:
                        cases.append((df, chan0, call, purpose))
    return cases


def fill_model(df, chan0, call, purpose):
    """The model of one case: (x, depth, margin, h, counts); counts holds the
    undecided share, the draws of retry depth >= 1 and >= 2, and the attempts
    rejected by 1 + c z <= 0."""
    st = {}
    x, depth, margin, h = chi2_rows(FILL_ROWS, chan0, FILL_N, df, FILL_SEED, call, purpose, stats=st)
    counts = {"undecided": float((margin < EPS).mean()), "depth1": int((depth >= 1).sum()),
              "depth2": int((depth >= 2).sum()), "neg_rejects": st.get("neg_rejects", 0)}
    return x, depth, margin, h, counts


def check_fill_counts(df, counts):
    """What a case must contain, from the model's own counts."""
    assert counts["undecided"] <= UNDECIDED_CAP, (df, counts)
    if df != 1.0:
        assert counts["depth1"] >= 1, (df, counts)
    if df == 0.5:
        assert counts["depth2"] >= 1 and counts["neg_rejects"] >= 1, (df, counts)
