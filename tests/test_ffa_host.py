"""The fast folding search without a GPU: the octave plan, the argument checks
of the three entry points, the NumPy restatement (tests/ffa_ref.py) against
properties of the definition, the clustering, and the CPU study that motivates
the stage.
"""
import re

import numpy as np
import pytest

from tests import ffa_ref as ref
from tests import kernel_harness as kh
from tests.kernel_harness import check_rejections, host_pointer

from psrsigsim_amd import _lib
from psrsigsim_amd.telescope import Backend


# ---------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------
def test_plan_by_hand():
    """fs = 10 kHz, T = 65536, B = 64, a = 100.5 and b = 499.3 samples:
    lf = floor(log2(100.5 / 64)) = 0, and 64 * 2^lf <= 499.3 up to lf = 2.
      lf 0: n 65536, p0 = max(64, floor(100.5)) = 100, last min(127, 500) = 127
      lf 1: n 32768, p0 64, last min(127, ceil(249.65)) = 127
      lf 2: n 16384, p0 64, last min(127, ceil(124.825)) = 125"""
    plan = Backend.ffa_plan(65536, 0.01, 0.01005, 0.04993, bins=64)
    assert [(o["lf"], o["n"], o["p0"], o["np"]) for o in plan] == [(0, 65536, 100, 28), (1, 32768, 64, 64),
                                                                   (2, 16384, 64, 62)]
    assert plan[0]["pmin"] == 100 / 1e4 and plan[0]["pmax"] == 128 / 1e4
    assert plan[2]["pmin"] == 64 * 4 / 1e4 and plan[2]["pmax"] == 126 * 4 / 1e4
    assert ref.plan_ref(65536, 1e4, 0.01005, 0.04993, 64) == [(0, 65536, 100, 28), (1, 32768, 64, 64),
                                                              (2, 16384, 64, 62)]
    # a = B exactly: one octave from lf = 0; a power-of-two a / B lands on its own octave
    assert [(o["lf"], o["p0"], o["np"]) for o in Backend.ffa_plan(65536, 0.01, 0.0256, 0.03, bins=256)] == \
        [(0, 256, 45)]
    assert [(o["lf"], o["n"], o["p0"], o["np"]) for o in Backend.ffa_plan(65536, 0.01, 0.1024, 0.1024, bins=256)] == \
        [(2, 16384, 256, 1)]
    # the default bins
    assert Backend.ffa_plan(1 << 20, 0.01, 0.05, 0.06)[0] == dict(lf=0, n=1 << 20, p0=500, np=12, pmin=0.05,
                                                                 pmax=512 / 1e4)


def test_plan_errors():
    for kw, word in ((dict(bins=8), "bins 8"), (dict(bins=4096), "bins 4096"), (dict(bins=64.5), "integers"),
                     (dict(pmin=0.006), "do not satisfy"),                    # a = 60 < B
                     (dict(pmax=0.01), "do not satisfy"),                     # b < a
                     (dict(pmin=float("nan")), "not finite"),
                     (dict(T=300, pmin=0.0128, pmax=0.02), "fewer than two periods of 100"),
                     (dict(T=1 << 28, bins=16, pmin=209.7152, pmax=209.7152), "beyond 2\\^16")):
        args = dict(T=65536, samprate=0.01, pmin=0.0128, pmax=0.05, bins=64)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            Backend.ffa_plan(**args)


def test_api_argument_errors():
    import torch
    from psrsigsim_amd.telescope import DedispersedPlane
    be = kh.backend()
    pl = DedispersedPlane(torch.zeros((3, 4096)), np.arange(3.0), np.zeros((3, 1), dtype=np.int32), 0.01, 1400.0, 0)
    with pytest.raises(ValueError, match="takes a DedispersedPlane"):
        be.ffa_snr(np.zeros((3, 4096)), 0.01, 0.02)
    for kw, word in ((dict(nwidths=0), "nwidths 0"), (dict(nwidths=12), "nwidths 12"), (dict(cell=24), "cell 24"),
                     (dict(stat_block=1), "stat_block"), (dict(bins=8), "bins 8"), (dict(mean=0.0), "both mean and std"),
                     (dict(max_bytes=1000), "max_bytes 1000")):
        with pytest.raises(ValueError, match=word):
            be.ffa_snr(pl, 0.0064, 0.01, **dict(dict(bins=64), **kw))
    with pytest.raises(ValueError, match="threshold"):
        be.ffa_search(pl, 0.0064, 0.01, threshold=0, bins=64)
    with pytest.raises(ValueError, match="freq_tol"):
        be.ffa_search(pl, 0.0064, 0.01, freq_tol=-1, bins=64)
    p = be._ffa_plan(pl, 0.0064, 0.01, bins=64)
    assert (p["ndm"], p["T"], p["fs"], p["nw"], p["cell"], p["threshold"]) == (3, 4096, 1e4, 6, 16, 8.0)
    assert [(o["lf"], o["p0"], o["np"]) for o in p["plan"]] == [(0, 64, 37)]
    # the chunks: whole trials while one fits, else runs of one trial's periods
    assert Backend._ffa_chunks(5, 1000, 10, 2 * 80000) == [(0, 2, 0, 10), (2, 4, 0, 10), (4, 5, 0, 10)]
    assert Backend._ffa_chunks(2, 1000, 10, 8000 * 4) == [(0, 1, 0, 4), (0, 1, 4, 8), (0, 1, 8, 10), (1, 2, 0, 4),
                                                           (1, 2, 4, 8), (1, 2, 8, 10)]


# ---------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------
def test_cabi_rejections():
    """NULL pointers and each out-of-range scalar return PSS_EINVAL with the
    argument named and no device touched."""
    p = host_pointer()
    L = _lib.load()
    # pss_ffa_scrunch(x, nser, T, ld, sub, lf, y, y_ld, stream)
    good = dict(x=p, nser=2, T=1000, ld=1000, sub=p, lf=2, y=p, y_ld=250)
    check_rejections(L.pss_ffa_scrunch, good,
                     ((dict(x=None), "x is NULL"), (dict(y=None), "y is NULL"), (dict(nser=0), "nser 0"),
                      (dict(lf=-1), "lf -1"), (dict(lf=17), "lf 17"), (dict(T=0, ld=0), "T 0"),
                      (dict(T=3, ld=3), "T 3"), (dict(ld=999), "ld 999"), (dict(y_ld=249), "y_ld 249"),
                      (dict(T=1 << 40, ld=1 << 40, lf=0, y_ld=1 << 40, nser=64), "workgroups")),
                     prefix="ffa_scrunch")
    # pss_ffa_transform(y, nser, n, ld, p0, np, out, work, stream)
    good = dict(y=p, nser=2, n=1000, ld=1000, p0=30, np=11, out=p, work=p)
    check_rejections(L.pss_ffa_transform, good,
                     ((dict(y=None), "y is NULL"), (dict(out=None), "out is NULL"), (dict(work=None), "work is NULL"),
                      (dict(nser=0), "nser 0"), (dict(p0=1), "p0 1"), (dict(np=0), "np 0"),
                      (dict(p0=990, np=12), "period 1001"),
                      (dict(n=10000, ld=10000, p0=4090, np=8), "period 4097"),
                      (dict(n=(1 << 28) + 1, ld=(1 << 28) + 1), "2^28"), (dict(ld=999), "ld 999"),
                      (dict(n=1 << 28, ld=1 << 28, p0=2, np=1, nser=100), "workgroups")),
                     prefix="ffa_transform")
    # pss_ffa_profile_search(prof, nser, n, p0, np, rstd, rm, nw, cell, snr, code, phase, out_ld, stream)
    good = dict(prof=p, nser=2, n=1000, p0=30, np=11, rstd=p, rm=p, nw=6, cell=16, snr=p, code=p, phase=p, out_ld=3)
    check_rejections(L.pss_ffa_profile_search, good,
                     ((dict(prof=None), "prof is NULL"), (dict(rstd=None), "rstd is NULL"), (dict(rm=None), "rm is NULL"),
                      (dict(snr=None), "snr is NULL"), (dict(code=None), "code is NULL"),
                      (dict(phase=None), "phase is NULL"), (dict(nser=-1), "nser -1"), (dict(p0=0), "p0 0"),
                      (dict(np=-3), "np -3"), (dict(np=1000), "period 1029"),
                      (dict(n=10000, p0=4096, np=2, out_ld=1), "period 4097"),
                      (dict(n=(1 << 28) + 1, out_ld=1 << 28), "2^28"), (dict(nw=0), "nw 0"), (dict(nw=12), "nw 12"),
                      (dict(cell=8), "cell 8"), (dict(cell=48), "cell 48"), (dict(cell=4096), "cell 4096"),
                      (dict(out_ld=2), "out_ld 2"),
                      (dict(n=1 << 28, p0=2, np=1, nser=1000, out_ld=1 << 23), "workgroups")),
                     prefix="ffa_profile_search")


def test_wiring():
    from psrsigsim_amd import build, telescope
    from psrsigsim_amd.telescope import backend
    assert "pss_ffa.hip" in build.UNITS and any(d.endswith("pss_ffa.hip") for d in build.DEPS)
    header = open(build.DEPS[-1]).read()
    for name, nargs in (("pss_ffa_scrunch", 9), ("pss_ffa_transform", 9), ("pss_ffa_profile_search", 14)):
        assert re.search(r"\bint\s+%s\s*\(" % name, header)
        assert len(_lib.EXPORTS[name][1]) == nargs and hasattr(_lib.load(), name)
    for name in ("FFAPlane", "FFACandidates", "Backend"):
        assert hasattr(telescope, name)
    assert issubclass(telescope.FFACandidates, telescope.PeriodCandidates)
    assert issubclass(Backend, backend.FFAStage) and hasattr(backend, "ffa_candidates_from_cells")


# ---------------------------------------------------------------------------
# the restatement against the definition
# ---------------------------------------------------------------------------
def test_scrunch_restatement():
    x = np.arange(1, 12, dtype=np.float32)[None, :]
    assert np.array_equal(ref.scrunch_ref(x, 0), x)
    assert np.array_equal(ref.scrunch_ref(x, 1)[0], [3, 7, 11, 15, 19])
    assert np.array_equal(ref.scrunch_ref(x, 2, sub=1.0)[0], [6, 22])         # (0+1)+(2+3), (4+5)+(6+7)
    assert np.array_equal(ref.scrunch_ref(x, 3)[0], [36])
    # the tree: ((a + b) + (c + d)), not a running sum
    v = np.array([[1e8, 1.0, -1e8, 1.0]], dtype=np.float32)
    assert ref.scrunch_ref(v, 2)[0, 0] == np.float32(np.float32(1e8) + np.float32(1)) + \
        np.float32(np.float32(-1e8) + np.float32(1))
    # octave from octave
    g = np.random.default_rng(1).standard_normal((2, 1003)).astype(np.float32)
    for lf in range(4):
        assert kh.same_bits(ref.scrunch_ref(ref.scrunch_ref(g, lf, 0.25), 1), ref.scrunch_ref(g, lf + 1, 0.25))


def test_transform_small_trees():
    rng = np.random.default_rng(2)
    r = rng.standard_normal((3, 7)).astype(np.float32)
    assert kh.same_bits(ref.transform_block(r[:1]), r[:1])                    # m = 1: the identity
    F = ref.transform_block(r[:2])                                            # m = 2
    assert kh.same_bits(F[0], r[0] + r[1]) and kh.same_bits(F[1], r[0] + np.roll(r[1], -1))
    # m = 3: h = 1, t = 2: i = 0; (j, b) = (0, 0), (1, 1), (1, 1) on Tl = F(1, 2)
    F = ref.transform_block(r)
    T0, T1 = r[1] + r[2], r[1] + np.roll(r[2], -1)
    assert [tuple(int(v[s]) for v in ref.rule(3)) for s in range(3)] == [(0, 0, 0), (0, 1, 1), (0, 1, 1)]
    assert kh.same_bits(F[0], r[0] + T0) and kh.same_bits(F[1], r[0] + np.roll(T1, -1))
    assert kh.same_bits(F[2], r[0] + np.roll(T1, -1))


@pytest.mark.parametrize("m,p", [(2, 5), (7, 3), (8, 16), (9, 2), (31, 37), (33, 64), (100, 19), (600, 4)])
def test_every_profile_sums_the_same_samples(m, p):
    """Integer data, exact sums: every profile holds every sample of the block
    once, and profile 0 is the plain fold."""
    x = np.random.default_rng(m * 100 + p).integers(-8, 8, size=(m, p)).astype(np.float32)
    F = ref.transform_block(x)
    assert F.shape == (m, p) and (F.sum(axis=1) == x.sum()).all()
    assert np.array_equal(F[0], x.sum(axis=0))
    # the last profile drifts one bin a row (b = h at s = m - 1 all the way down)
    assert np.array_equal(F[m - 1], sum(np.roll(x[r], -r) for r in range(m)))


def test_rule_bounds_and_subtrees_fit():
    """0 <= i_s < h, 0 <= j_s < t for every node size; and the nodes of the
    depth the kernel fuses at hold at most LDS_FLOATS floats, at least two rows
    wherever the tree has two."""
    for m in list(range(2, 300)) + [511, 512, 513, 4095, 4097, 40000, (1 << 27) - 1]:
        i, j, b = ref.rule(m)
        h = m // 2
        assert i.min() == 0 and i.max() == max(h - 1, 0) and j.min() == 0 and j.max() == m - h - 1
        assert b.min() == 0 and b.max() == h and (np.diff(i) >= 0).all() and (np.diff(b) >= 0).all()

    def sizes(m, d):
        return [m] if d == 0 or m == 1 else sizes(m // 2, d - 1) + sizes(m - m // 2, d - 1)
    for m, p in ((1, 4096), (2, 4096), (3, 4096), (3, 2731), (33, 37), (600, 64), (4091, 256), (4096, 2), (9999, 3),
                 (257, 511)):
        d = ref.fuse_depth(m, p)
        assert max(sizes(m, d)) * p <= ref.LDS_FLOATS and (d == 0 or max(sizes(m, d - 1)) * p > ref.LDS_FLOATS)
        assert d <= max(ref.depth(m) - 1, 0) and len(sizes(m, d)) == 1 << d


@pytest.mark.parametrize("n,p", [(1000, 37), (4096, 64), (5000, 100), (777, 19)])
def test_impulse_train_lands_in_its_profile(n, p):
    """Impulses at floor(k P + 5.5), P = p + s / (m - 1), for every s: profile s
    of the restatement holds at least 0.68 of them in two adjacent bins and at
    least 0.94 in four (the minima over these shapes, both at (5000, 100))."""
    m = n // p
    worst2 = worst4 = 1.0
    for s in range(m):
        P = p + s / (m - 1.0)
        t = np.floor(np.arange(int(n / P) + 2) * P + 5.5).astype(np.int64)
        x = np.zeros(m * p, dtype=np.float32)
        x[t[t < m * p]] = 1.0
        prof = ref.transform_block(x.reshape(m, p))[s]
        assert prof.sum() == x.sum()
        two = prof + np.roll(prof, -1)
        four = two + np.roll(two, -2)
        worst2, worst4 = min(worst2, two.max() / x.sum()), min(worst4, four.max() / x.sum())
    print("(%d, %d): two bins %.4f, four bins %.4f" % (n, p, worst2, worst4))
    assert worst2 >= 0.68 and worst4 >= 0.94


def test_z_is_unit_variance_on_noise():
    """z of the one-bin box (k = 0) over every profile of unit-normal noise,
    n = 65536, p = 250, rm = 1 / sqrt(m): each is a sum of m samples over
    sqrt(m).  Measured standard deviation 1.0043 (65500 values of 65500
    samples: neighbouring profiles share most of their terms, so the estimate
    is good to about 1 / sqrt(2 * 250) = 0.045 at worst; the bound is 3 %)."""
    n, p = 65536, 250
    m = n // p
    x = np.random.default_rng(0).standard_normal(n).astype(np.float32)
    F = ref.transform_block(x[:m * p].reshape(m, p))
    z = (F * np.float32(1.0)) * np.float32(1.0 / np.sqrt(m))
    print("std of z at k = 0:", z.std(), "mean", z.mean())
    assert abs(z.std() - 1.0) < 0.03
    # and the search's own z at k = 0 is that number
    bz, bk, bf = ref.best_per_profile(F, np.float32(1.0 / np.sqrt(m)), 1)
    assert np.array_equal(bz, z.max(axis=1)) and (bk == 0).all() and np.array_equal(bf, z.argmax(axis=1))


def test_profile_search_restatement_by_hand():
    """One block, n = 12, p = 6, m = 2, two "cells" of one profile each (the
    restatement takes any cell).  Row 0 = 0 0 5 0 0 3, row 1 = 4 0 0 0 0 4:
      k 0: z = S            best row 0: 5 at f 2; row 1: 4 at f 0
      k 1: S + roll(-1)     row 0: 0 5 5 0 3 3 -> 5 sqrt(1/2) = 3.54; row 1: the box
                            (5, 0) that wraps = 8 -> 5.657 at f 5
      k 2 needs 2^3 <= 6: not valid."""
    prof = np.array([[[0, 0, 5, 0, 0, 3, 4, 0, 0, 0, 0, 4]]], dtype=np.float32)
    snr, code, phase = ref.profile_search_ref(prof, 12, 6, 1, 1.0, 1.0, 5, 1)
    assert snr.shape == (1, 1, 2)
    assert snr[0, 0, 0] == 5.0 and code[0, 0, 0] == 0 and phase[0, 0, 0] == 2
    assert snr[0, 0, 1] == np.float32(8.0) * ref.psr.coef(1) and code[0, 0, 1] == 1 << 16 and phase[0, 0, 1] == 5
    # both profiles in one cell: the wider box of row 1 wins; g scales z by one rounded product
    snr, code, phase = ref.profile_search_ref(prof, 12, 6, 1, 0.5, 3.0, 5, 2)
    assert snr[0, 0, 0] == np.float32(np.float32(8.0) * ref.psr.coef(1)) * np.float32(1.5)
    assert code[0, 0, 0] == (1 << 16) | 1 and phase[0, 0, 0] == 5
    shift, wl = ref.decode(code, 2)
    assert shift[0, 0, 0] == 1 and wl[0, 0, 0] == 1


# ---------------------------------------------------------------------------
# clustering and order
# ---------------------------------------------------------------------------
def test_candidates_cluster_and_order():
    from psrsigsim_amd.telescope.backend import ffa_candidates_from_cells, FFA_DTYPE
    # columns: (octave, lf, p, m, q); T = 65536 at 10 kHz
    columns = np.array([(0, 0, 250, 262, 6), (0, 0, 250, 262, 5), (0, 0, 251, 261, 0), (1, 1, 250, 131, 0)])
    T, fs = 65536, 1e4
    # cells: (snr, trial, column, shift, width_log2, phase)
    cells = [(9.0, 3, 0, 96, 2, 10),      # P = 250 + 96 / 261 = 250.368: F = round(16 T / P) = 4188
             (12.0, 4, 0, 97, 2, 11),     # a neighbouring trial, F 4188: the same cluster, its best
             (8.5, 4, 1, 95, 1, 9),       # F 4188
             (12.0, 6, 0, 97, 2, 11),     # trial 6: two trials away, its own cluster, ties in snr with the first
             (10.0, 4, 2, 0, 0, 3),       # P = 251: F 4178, 10 sixteenths away: friends at freq_tol 1 (16)
             (11.0, 4, 3, 20, 3, 7)]      # P = 2 (250 + 20 / 130) = 500.31: F 2096, the half harmonic stays apart
    a = [np.array(c) for c in zip(*cells)]
    got = ffa_candidates_from_cells(a[0], a[1], a[2], a[3], a[4], a[5], columns, T, fs, np.arange(8) * 5.0)
    assert got.dtype == FFA_DTYPE and len(got) == 3
    assert [(float(g["snr"]), int(g["dm_index"]), int(g["ncells"])) for g in got] == [(12.0, 4, 4), (12.0, 6, 1),
                                                                                   (11.0, 4, 1)]
    g = got[0]
    assert g["period"] == (250 + 97 / 261.0) / fs and g["freq"] == 1.0 / g["period"] and g["dm"] == 20.0
    assert (g["width"], g["width_sec"], g["phase"], g["bins"], g["octave"], g["shift"]) == (4, 4 / fs, 11, 250, 0, 97)
    h = got[2]
    assert h["period"] == (250 + 20 / 130.0) * 2 / fs and h["width"] == 8 and h["width_sec"] == 16 / fs
    assert h["octave"] == 1 and h["bins"] == 250
    # a tighter tolerance separates P = 251; dm_tol 2 joins trial 6
    tight = ffa_candidates_from_cells(a[0], a[1], a[2], a[3], a[4], a[5], columns, T, fs, np.arange(8) * 5.0,
                                      freq_tol=0.5)
    assert sorted(int(c) for c in tight["ncells"]) == [1, 1, 1, 3]
    wide = ffa_candidates_from_cells(a[0], a[1], a[2], a[3], a[4], a[5], columns, T, fs, np.arange(8) * 5.0, dm_tol=2)
    assert sorted(int(c) for c in wide["ncells"]) == [1, 5] and int(wide[0]["dm_index"]) == 4
    # the order: snr descending, then dm_index, then period
    assert list(got["snr"]) == sorted(got["snr"], reverse=True)
    none = ffa_candidates_from_cells(*([np.zeros(0)] * 6), columns, T, fs, np.arange(8) * 5.0)
    assert len(none) == 0 and none.dtype == FFA_DTYPE
    # the restatement's clustering (all pairs) agrees
    maps = dict(snr=np.full((8, 4), -np.inf, dtype=np.float32), period=np.ones((8, 4)), phase=np.zeros((8, 4), int),
                shift=np.zeros((8, 4), int), width_log2=np.zeros((8, 4), int), columns=columns)
    for s, j, c, sh, wl, f in cells[:3] + cells[4:]:
        if maps["snr"][j, c] < s:
            maps["snr"][j, c], maps["shift"][j, c], maps["width_log2"][j, c], maps["phase"][j, c] = s, sh, wl, f
            maps["period"][j, c] = (columns[c, 2] + sh / (columns[c, 3] - 1.0)) * 2.0 ** columns[c, 1] / fs
    want = ref.candidates_ref(maps, T, fs, 8.0)
    assert [(w[0], w[1], w[8]) for w in want] == [(12.0, 4, 4), (11.0, 4, 1)]


# ---------------------------------------------------------------------------
# the study behind the stage
# ---------------------------------------------------------------------------
@kh.once
def study(seed):
    """Unit-normal noise from default_rng(seed), 65536 samples, plus a pulse
    train of period 250.37 samples, width 3, amplitude 0.55 (pulse k fills the
    three samples from floor(250.37 k + 0.5)); the best (z, p, s, k) over the
    base periods 247 .. 253 with rstd 1 and rm = 1 / sqrt(m)."""
    n, P = 65536, 250.37
    x = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    for t0 in np.floor(np.arange(int(n / P) + 1) * P + 0.5).astype(np.int64):
        x[t0:t0 + 3] += np.float32(0.55)
    best = None
    for p in range(247, 254):
        m = n // p
        z, k, f = ref.best_per_profile(ref.transform_block(x[:m * p].reshape(m, p)), np.float32(1 / np.sqrt(m)), 6)
        s = int(np.argmax(z))
        if best is None or z[s] > best[0]:
            best = (float(z[s]), p, s, int(k[s]))
    return best


@pytest.mark.parametrize("seed", range(6))
def test_cpu_study(seed):
    """The best profile lies at base period 250, shift 96 or 97 of 262 (250.368
    to 250.372 samples), width 4, with z between 12 and 14.1, in all six seeds
    (here: shift 97 in all six, z 12.56 .. 13.98)."""
    z, p, s, k = study(seed)
    print(seed, z, p, s, k)
    assert (p, k) == (250, 2) and s in (96, 97) and 12.0 <= z <= 14.1
