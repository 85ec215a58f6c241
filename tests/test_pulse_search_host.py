"""Host side of the single-pulse search (no GPU): every Python-level rejection
(nothing reaches the device), the C ABI's argument checks, which precede any
launch, the friends-of-friends clustering against an all-pairs restatement,
the candidates' order, and the float32 restatement of the kernel itself
(tests/pulse_search_ref.py) on a hand-computed row."""
import numpy as np
import pytest

from psrsigsim_amd import _lib
from tests import pulse_search_ref as ref
from tests.kernel_harness import backend as _backend, check_rejections, host_pointer


class _StubData(object):
    """Stands in for the plane's device tensor: only its shape may be read."""

    def __init__(self, ndm, T):
        self.shape = (ndm, T)

    def __getattr__(self, name):
        raise AssertionError("the device buffer was touched (%s)" % name)


def _plane(ndm=13, T=15635):
    from psrsigsim_amd.telescope import DedispersedPlane
    return DedispersedPlane(_StubData(ndm, T), np.arange(ndm) * 5.0, np.zeros((ndm, 4), dtype=np.int32), 0.01,
                            1593.75, 749)


def test_rejections_never_reach_the_device(monkeypatch):
    from psrsigsim_amd import _engine

    def boom(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_engine, "to_dev", boom)
    monkeypatch.setattr(_engine, "execute", boom)
    be = _backend()
    pl = _plane()
    both = (be.boxcar_snr, be.single_pulse_search)
    for fn in both:
        with pytest.raises(ValueError, match="DedispersedPlane"):
            fn(np.zeros((3, 100), dtype=np.float32))
        with pytest.raises(ValueError, match="DedispersedPlane"):
            fn(None)
        for bad in (0, 14, -1, 2.5, "x", None):
            with pytest.raises(ValueError, match="nwidths|integers"):
                fn(pl, nwidths=bad)
        for bad in (0, 8, 24, 4096, -32, 33, 32.5):
            with pytest.raises(ValueError, match="cell|integers"):
                fn(pl, cell=bad)
        for bad in (1, 0, -5):
            with pytest.raises(ValueError, match="stat_block"):
                fn(pl, stat_block=bad)
        with pytest.raises(ValueError, match="mean has 12 entries for 13"):
            fn(pl, mean=np.zeros(12), std=np.ones(13))
        with pytest.raises(ValueError, match="std has 14 entries for 13"):
            fn(pl, mean=0.0, std=np.ones(14))
        with pytest.raises(ValueError, match="std has 2x13 entries"):
            fn(pl, mean=0.0, std=np.ones((2, 13)))
        for bad in (np.nan, np.inf):
            with pytest.raises(ValueError, match="mean has an entry that is not finite"):
                fn(pl, mean=bad, std=1.0)
            with pytest.raises(ValueError, match="std has an entry that is not finite"):
                fn(pl, mean=0.0, std=bad)
        m = np.zeros(13)
        m[7] = np.nan
        with pytest.raises(ValueError, match="mean has an entry that is not finite"):
            fn(pl, mean=m, std=np.ones(13))
        s = np.ones(13)
        s[3] = 0.0
        with pytest.raises(ValueError, match="std has an entry <= 0"):
            fn(pl, mean=0.0, std=s)
        with pytest.raises(ValueError, match="std has an entry <= 0"):
            fn(pl, mean=0.0, std=-1.0)
        with pytest.raises(ValueError, match="both mean and std"):
            fn(pl, mean=0.0)
    for bad in (0.0, -6.0, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="threshold"):
            be.single_pulse_search(pl, threshold=bad)
    with pytest.raises(ValueError, match="dm_tol"):
        be.single_pulse_search(pl, dm_tol=-1)
    with pytest.raises(ValueError, match="time_tol"):
        be.single_pulse_search(pl, time_tol=-1)
    with pytest.raises(ValueError, match="max_cells"):
        be.single_pulse_search(pl, max_cells=-1)
    # the plan of a valid call
    plan = be._search_plan(pl, nwidths=13, cell=2048, threshold=7, dm_tol=0, time_tol=5, max_cells=10,
                           mean=1.5, std=np.full(13, 2.0), stat_block=2)
    assert plan[:8] == (13, 15635, 13, 2048, 7.0, 0, 5, 10) and plan[10] == 2
    assert plan[8].dtype == np.float64 and np.array_equal(plan[8], np.full(13, 1.5))
    assert np.array_equal(plan[9], np.full(13, 2.0))
    plan = be._search_plan(pl)
    assert plan == (13, 15635, 8, 32, 6.0, 1, 0, 1 << 20, None, None, 1024)


def test_cabi_rejections():
    """NULL pointers and each out-of-range scalar return PSS_EINVAL with the
    argument named and no device touched."""
    p = host_pointer()
    # pss_boxcar_search(plane, ndm, T, ld, mean, rstd, nw, cell, snr, code, out_ld, stream)
    good = dict(plane=p, ndm=3, T=1000, ld=1000, mean=p, rstd=p, nw=8, cell=32, snr=p, code=p, out_ld=32)
    check_rejections(_lib.load().pss_boxcar_search, good,
                    ((dict(plane=None), "plane"), (dict(mean=None), "mean"), (dict(rstd=None), "rstd"),
                     (dict(snr=None), "snr"), (dict(code=None), "code"),
                     (dict(ndm=0), "ndm 0"), (dict(ndm=-2), "ndm -2"),
                     (dict(T=0), "T 0"), (dict(T=-1, ld=0), "T -1"),
                     (dict(ld=999), "ld 999"),
                     (dict(nw=0), "nw 0"), (dict(nw=14), "nw 14"), (dict(nw=-1), "nw -1"),
                     (dict(cell=8), "cell 8"), (dict(cell=0), "cell 0"), (dict(cell=48), "cell 48"),
                     (dict(cell=4096), "cell 4096"), (dict(cell=-32), "cell -32"),
                     (dict(out_ld=31), "out_ld 31"), (dict(cell=16, out_ld=62), "out_ld 62"),
                     (dict(T=1025, ld=1025, out_ld=32), "out_ld 32"),
                     # the launch grid: ceil(T / 2048) * ndm workgroups in 31 bits
                     (dict(T=1 << 40, ld=1 << 40, out_ld=1 << 40, ndm=64), "workgroups")), prefix="boxcar_search")


def test_wiring():
    from psrsigsim_amd import build, telescope
    assert "pss_boxsearch.hip" in build.UNITS
    assert any(d.endswith("pss_boxsearch.hip") for d in build.DEPS)
    assert "pss_boxcar_search" in _lib.EXPORTS and hasattr(_lib.load(), "pss_boxcar_search")
    for name in ("BoxcarPlane", "PulseCandidates", "DedispersedPlane", "Backend"):
        assert hasattr(telescope, name)


# ---------------------------------------------------------------------------
# the restatement itself
# ---------------------------------------------------------------------------
def test_restatement_on_a_hand_computed_row():
    """x = 1 -2 3 3 0 -1 2 5, mean 0, rstd 1, three widths, two "cells" of 4
    (the restatement takes any cell; the kernel's start at 16):
      S_0 = 1 -2  3  3  0 -1  2  5                   z_0 = S_0
      S_1 = -1  1  6  3 -1  1  7        (7 boxes)    z_1 = S_1 * fp32(sqrt 2) / 2
      S_2 =  5  4  5  4  6              (5 boxes)    z_2 = S_2 / 2
    per time the best (z, k): t0 (2.5, 2), t1 (2, 2), t2 (6 r, 1), t3 (3, 0) [3 > 3 r = 2.12],
    t4 (3, 2), t5 (r, 1), t6 (7 r, 1), t7 (5, 0), with r = fp32(sqrt 2) / 2."""
    x = np.array([[1, -2, 3, 3, 0, -1, 2, 5]], dtype=np.float32)
    r = np.float32(ref.SQRT2_F32 * np.float32(0.5))
    assert ref.coef(0) == 1.0 and ref.coef(1) == r and ref.coef(2) == 0.5 and ref.coef(3) == np.float32(r * 0.5)
    assert ref.coef(12) == np.float32(2.0 ** -6) and ref.coef(11) == np.float32(ref.SQRT2_F32 * 2.0 ** -6)
    bz, bk = ref.best_per_time(x[0], 0.0, 1.0, 3)
    assert np.array_equal(bz, np.array([2.5, 2, np.float32(6) * r, 3, 3, r, np.float32(7) * r, 5], dtype=np.float32))
    assert np.array_equal(bk, [2, 2, 1, 0, 2, 1, 1, 0])
    snr, code = ref.boxcar_ref(x, 0.0, 1.0, 3, 4)
    assert snr.dtype == np.float32 and code.dtype == np.int32
    assert np.array_equal(snr, [[np.float32(6) * r, 5.0]])
    assert np.array_equal(code, [[(1 << 16) | 2, (0 << 16) | 3]])
    time, wl = ref.decode(code, 4)
    assert np.array_equal(time, [[2, 7]]) and np.array_equal(wl, [[1, 0]])
    # mean and rstd enter as y = x - mean, c = a_k * rstd: twice the scale, same winners
    snr2, code2 = ref.boxcar_ref(x * 2 + 3, 3.0, 0.5, 3, 4)
    assert np.array_equal(snr2, snr) and np.array_equal(code2, code)
    # ties: the narrower width, then the earlier time; an all-NaN cell gives -inf, code 0
    y = np.array([[0, 2, 0, 2, np.nan, np.nan, np.nan, np.nan, 4, 0, 0, 0]], dtype=np.float32)
    snr, code = ref.boxcar_ref(y, 0.0, 1.0, 3, 4)
    #  cell 0: z_2 = (0+2+0+2)/2 = 2 at t = 0, z_0 = 2 at t = 1 and 3 -> width 1, t = 1
    #  cell 1: every box from t = 4 .. 7 of any width holds a NaN
    #  cell 2: widths 1, 2 and 4 at t = 8 give 4, 2.83, 2
    assert np.array_equal(snr, np.array([[2.0, -np.inf, 4.0]], dtype=np.float32))
    assert np.array_equal(code, [[1, 0, 0]])
    # widths that do not fit do not exist: T = 3 has no width 4
    bz, bk = ref.best_per_time(np.array([1, 1, 1], dtype=np.float32), 0.0, 1.0, 5)
    assert np.array_equal(bk, [1, 1, 0]) and bz[2] == 1.0


def test_block_median_statistics():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 1000)) * np.array([[1.0], [2.0], [0.5]]) + np.array([[10.0], [0.0], [-3.0]])
    x[0, 100:140] += 50.0                      # a pulse in one block moves neither median
    mean, var = ref.block_median_stats(x, 100)
    assert np.allclose(mean, [10, 0, -3], atol=0.3) and np.allclose(np.sqrt(var), [1, 2, 0.5], rtol=0.2)
    # the lower median of an even count; trailing samples do not enter
    z = np.concatenate([np.full(10, v, dtype=np.float64) for v in (4.0, 1.0, 3.0, 2.0)] + [np.full(7, 99.0)])[None, :]
    mean, var = ref.block_median_stats(z, 10)
    assert mean[0] == 2.0 and var[0] == 0.0
    m32, r32 = ref.stats_to_f32(mean, var)
    assert m32[0] == 2.0 and r32[0] == 0.0 and r32.dtype == np.float32


# ---------------------------------------------------------------------------
# clustering and candidates
# ---------------------------------------------------------------------------
def _same_partition(a, b):
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


@pytest.mark.parametrize("dm_tol", [0, 1, 2])
@pytest.mark.parametrize("time_tol", [0, 5])
def test_sweep_equals_all_pairs(dm_tol, time_tol):
    from psrsigsim_amd.telescope.backend import cluster_cells, candidates_from_cells
    rng = np.random.default_rng(1000 + 10 * dm_tol + time_tol)
    n = 2000
    j = rng.integers(0, 40, size=n)
    t = rng.integers(0, 20000, size=n)
    w = 1 << rng.integers(0, 8, size=n)
    snr = rng.integers(12, 40, size=n).astype(np.float32) / 2          # many equal S/N: the tie-breaks matter
    got = cluster_cells(j, t, w, dm_tol, time_tol)
    want = ref.cluster_all_pairs(j, t, w, dm_tol, time_tol)
    nclusters = len(set(want.tolist()))
    assert 20 < nclusters < n - 20, nclusters                          # neither trivial partition
    assert np.array_equal(got, want)                                   # both label by the smallest member
    assert _same_partition(got, want)
    cand = candidates_from_cells(snr, j, t, w, np.arange(40) * 2.5, 0.01, dm_tol, time_tol)
    expect = ref.candidates_ref(snr, j, t, w, want)
    assert len(cand) == len(expect) == nclusters
    got_rows = [(float(c["snr"]), int(c["dm_index"]), int(c["time"]), int(c["width"]), int(c["ncells"]))
                for c in cand]
    assert got_rows == expect
    assert int(cand["ncells"].sum()) == n


def test_a_long_chain_is_one_cluster():
    """50 000 touching boxes in one trial: one cluster, in well under all-pairs time."""
    from psrsigsim_amd.telescope.backend import cluster_cells, candidates_from_cells
    n = 50000
    t = np.arange(n, dtype=np.int64) * 4
    perm = np.random.default_rng(3).permutation(n)
    labels = cluster_cells(np.full(n, 7)[perm], t[perm], np.full(n, 4), 1, 0)
    assert (labels == 0).all()
    # one sample of gap at time_tol 0 splits it; time_tol 1 joins it again
    t2 = t.copy()
    t2[n // 2:] += 1
    assert len(set(cluster_cells(np.full(n, 7), t2, np.full(n, 4), 1, 0).tolist())) == 2
    assert len(set(cluster_cells(np.full(n, 7), t2, np.full(n, 4), 1, 1).tolist())) == 1
    snr = np.full(n, 8.0, dtype=np.float32)
    cand = candidates_from_cells(snr[perm], np.full(n, 7), t[perm], np.full(n, 4), np.arange(13) * 5.0, 0.01)
    assert len(cand) == 1 and cand[0]["ncells"] == n and cand[0]["time"] == 0 and cand[0]["dm"] == 35.0


def test_friend_rule_and_output_order():
    from psrsigsim_amd.telescope.backend import cluster_cells, candidates_from_cells, CANDIDATE_DTYPE
    # boxes [0,4) and [4,6) touch; [7,8) is one sample away; trial 3 is two trials from 1
    j = np.array([1, 1, 1, 3, 2])
    t = np.array([0, 4, 7, 0, 100])
    w = np.array([4, 2, 1, 4, 8])
    assert cluster_cells(j, t, w, 1, 0).tolist() == [0, 0, 2, 3, 4]
    assert cluster_cells(j, t, w, 1, 1).tolist() == [0, 0, 0, 3, 4]
    assert cluster_cells(j, t, w, 2, 0).tolist() == [0, 0, 2, 0, 4]
    assert cluster_cells(j, t, w, 0, 10 ** 6).tolist() == [0, 0, 0, 3, 4]
    # a cell of trial 2 that overlaps both bridges trials 1 and 3 at dm_tol 1
    assert cluster_cells(np.append(j, 2), np.append(t, 2), np.append(w, 1), 1, 0).tolist() == [0, 0, 2, 0, 4, 0]
    # the candidate of a cluster: the largest snr, then the lower trial, then the earlier time
    snr = np.array([9, 9, 7, 9, 9], dtype=np.float32)
    c = candidates_from_cells(snr, j, t, w, np.arange(5) * 10.0, 0.5, dm_tol=1, time_tol=1)
    assert c.dtype == CANDIDATE_DTYPE
    # clusters {0, 1, 2}, {3}, {4}, all at snr 9: ordered by (dm_index, time, width)
    assert c["dm_index"].tolist() == [1, 2, 3] and c["time"].tolist() == [0, 100, 0]
    assert c["width"].tolist() == [4, 8, 4] and c["ncells"].tolist() == [3, 1, 1]
    assert c["dm"].tolist() == [10.0, 20.0, 30.0]
    assert c["t_sec"].tolist() == [(0 + 2.0) / 0.5e6, (100 + 4.0) / 0.5e6, (0 + 2.0) / 0.5e6]
    # snr descending comes first
    c = candidates_from_cells(np.array([6, 6.5, 7, 8, 6], dtype=np.float32), j, t, w, np.arange(5) * 10.0, 0.5, 0, 0)
    assert c["snr"].tolist() == [8.0, 7.0, 6.5, 6.0] and c["ncells"].tolist() == [1, 1, 2, 1]
    assert c["time"].tolist() == [0, 7, 4, 100]
    # nothing above the threshold
    e = candidates_from_cells(np.zeros(0, dtype=np.float32), [], [], [], np.arange(5) * 10.0, 0.5)
    assert len(e) == 0 and e.dtype == CANDIDATE_DTYPE


def test_pulse_candidates_container():
    from psrsigsim_amd.telescope import PulseCandidates
    from psrsigsim_amd.telescope.backend import candidates_from_cells
    arr = candidates_from_cells(np.array([8, 7], dtype=np.float32), [2, 5], [10, 900], [4, 1], np.arange(6) * 5.0, 0.01)
    pc = PulseCandidates(arr, "cells", 6.0)
    assert len(pc) == 2 and pc.cells == "cells" and pc.threshold == 6.0
    assert pc.snr.tolist() == [8.0, 7.0] and pc.dm.tolist() == [10.0, 25.0] and pc.width.tolist() == [4, 1]
    assert pc[1]["time"] == 900 and pc.array is arr
    with pytest.raises(AttributeError):
        pc.nothing


def test_max_cells_names_the_threshold(monkeypatch):
    """More cells above the threshold than max_cells: a ValueError that names
    the threshold (boxcar_snr stubbed: no device)."""
    import torch
    from psrsigsim_amd.telescope import Backend, BoxcarPlane
    pl = _plane(ndm=2, T=64)
    snr = torch.tensor([[7.0, 3.0], [8.0, 9.0]])
    time = torch.tensor([[3, 40], [5, 33]])
    wl = torch.tensor([[0, 1], [2, 0]], dtype=torch.int32)
    cells = BoxcarPlane(snr, time, wl, None, None, None, 32, pl)
    monkeypatch.setattr(Backend, "boxcar_snr", lambda self, plane, **kw: cells)
    be = _backend()
    with pytest.raises(ValueError, match=r"3 cells at or above threshold 6 exceed max_cells 2"):
        be.single_pulse_search(pl, threshold=6.0, max_cells=2)
    got = be.single_pulse_search(pl, threshold=6.0, max_cells=3, dm_tol=0)
    assert got.cells is cells and len(got) == 3
    assert got.snr.tolist() == [9.0, 8.0, 7.0] and got.dm_index.tolist() == [1, 1, 0]
    assert got.time.tolist() == [33, 5, 3] and got.width.tolist() == [1, 4, 1]
    # at dm_tol 1 the boxes [3, 4) of trial 0 and [5, 9) of trial 1 stay apart, at time_tol 1 they join
    assert len(be.single_pulse_search(pl, threshold=6.0, dm_tol=1, time_tol=1)) == 2
