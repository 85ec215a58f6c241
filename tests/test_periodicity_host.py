"""Host side of the periodicity search (no GPU): every Python-level rejection
(nothing reaches the device), ``Backend.fft_length`` against brute force, the
C ABI's argument checks, which precede any launch, the clustering on the
fundamental and the candidate table against an all-pairs restatement, the
false-alarm probability, and the float32 restatement of the kernel itself
(tests/periodicity_ref.py) on a hand-computed row."""
import numpy as np
import pytest

from psrsigsim_amd import _lib
from tests import periodicity_ref as ref
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
    for fn in (be.harmonic_snr, be.periodicity_search):
        with pytest.raises(ValueError, match="DedispersedPlane"):
            fn(np.zeros((3, 100), dtype=np.float32))
        with pytest.raises(ValueError, match="DedispersedPlane"):
            fn(None)
        for bad in (0, 3, 32, -1, 2.5, "x", None):
            with pytest.raises(ValueError, match="nharm|integers"):
                fn(pl, nharm=bad)
        for bad in (0, 8, 24, 4096, -32, 33, 32.5):
            with pytest.raises(ValueError, match="cell|integers"):
                fn(pl, cell=bad)
        for bad in (1, 0, -5):
            with pytest.raises(ValueError, match="stat_block"):
                fn(pl, stat_block=bad)
        for bad in (0, 1, 7, -8, 1001, 1 << 29, 100.5):
            with pytest.raises(ValueError, match="nfft|integers"):
                fn(pl, nfft=bad)
        for bad in (-1.0, np.nan, np.inf, "x"):
            with pytest.raises(ValueError, match="fmin"):
                fn(pl, fmin=bad)
        with pytest.raises(ValueError, match="max_bytes 1000 is below one trial"):
            fn(pl, max_bytes=1000)
        with pytest.raises(ValueError, match="mean has 12 entries for 13"):
            fn(pl, mean=np.zeros(12), std=np.ones(13))
        with pytest.raises(ValueError, match="std has 2x13 entries"):
            fn(pl, mean=0.0, std=np.ones((2, 13)))
        with pytest.raises(ValueError, match="mean has an entry that is not finite"):
            fn(pl, mean=np.nan, std=1.0)
        with pytest.raises(ValueError, match="std has an entry <= 0"):
            fn(pl, mean=0.0, std=0.0)
        with pytest.raises(ValueError, match="both mean and std"):
            fn(pl, std=1.0)
        with pytest.raises(ValueError, match="spectrum has the shape 12x7501 for 13"):
            fn(pl, spectrum=_StubData(12, 7501))
        with pytest.raises(ValueError, match="spectrum has 7501 bins, nfft 15552 gives 7777"):
            fn(pl, nfft=15552, spectrum=_StubData(13, 7501))
    with pytest.raises(ValueError, match="DedispersedPlane"):
        be.dm_spectrum(None)
    with pytest.raises(ValueError, match="nfft"):
        be.dm_spectrum(pl, nfft=1001)
    for bad in (0.0, -6.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="threshold"):
            be.periodicity_search(pl, threshold=bad)
    with pytest.raises(ValueError, match="dm_tol"):
        be.periodicity_search(pl, dm_tol=-1)
    with pytest.raises(ValueError, match="freq_tol"):
        be.periodicity_search(pl, freq_tol=-0.5)
    with pytest.raises(ValueError, match="max_cells"):
        be.periodicity_search(pl, max_cells=-1)
    # the plan of a valid call: T = 15635 -> nfft 15552 = 2^6 3^5, df = 1e4 / nfft Hz
    p = be._harmonic_plan(pl)
    assert (p["ndm"], p["T"], p["nl"], p["cell"], p["nfft"], p["nbin"], p["n_used"]) == (13, 15635, 5, 32, 15552,
                                                                                        7776, 15552)
    assert p["df"] == 1e4 / 15552 and p["kmin"] == 1 and p["threshold"] == 10.0 and p["chunk"] == 13
    assert p["mean"] is None and p["std"] is None and p["max_cells"] == 1 << 20 and p["stat_block"] == 1024
    p = be._harmonic_plan(pl, nharm=4, cell=2048, nfft=40000, fmin=2.0, threshold=12, dm_tol=0, freq_tol=0.0625,
                          max_cells=5, mean=1.5, std=np.full(13, 2.0), stat_block=2, max_bytes=3 * 20001 * 8 + 7)
    assert (p["nl"], p["cell"], p["nfft"], p["nbin"], p["n_used"]) == (3, 2048, 40000, 20000, 15635)
    assert p["df"] == 0.25 and p["kmin"] == 8 and p["chunk"] == 3 and p["freq_tol"] == 0.0625
    assert p["mean"].dtype == np.float64 and np.array_equal(p["mean"], np.full(13, 1.5))
    assert be._harmonic_plan(pl, nfft=40000, fmin=2.01)["kmin"] == 9
    assert be._harmonic_plan(pl, fmin=0.0)["kmin"] == 1
    assert [be._harmonic_plan(pl, nharm=h)["nl"] for h in (1, 2, 4, 8, 16)] == [1, 2, 3, 4, 5]
    # a given spectrum fixes nfft
    assert be._harmonic_plan(pl, spectrum=_StubData(13, 7501))["nfft"] == 15000


def test_fft_length_equals_brute_force():
    from psrsigsim_amd.telescope import Backend
    for T in list(range(2, 700)) + [1 << 20, (1 << 20) - 1, (1 << 20) + 1, 1046607, 40921, 15635, 3 ** 9, 5 ** 8 * 2]:
        assert Backend.fft_length(T) == ref.fft_length_ref(T), T
    assert Backend.fft_length(2) == 2 and Backend.fft_length(3) == 2 and Backend.fft_length(1 << 20) == 1 << 20
    assert Backend.fft_length(1046607) == 1036800                       # 2^9 3^4 5^2
    for bad in (1, 0, -4):
        with pytest.raises(ValueError, match="fft_length"):
            Backend.fft_length(bad)


def test_cabi_rejections():
    """NULL pointers and each out-of-range scalar return PSS_EINVAL with the
    argument named and no device touched."""
    p = host_pointer()
    # pss_harmonic_search(spec, ndm, nbin, ld, scale, nl, kmin, cell, snr, code, out_ld, work, stream)
    good = dict(spec=p, ndm=3, nbin=1000, ld=1001, scale=p, nl=5, kmin=1, cell=32, snr=p, code=p, out_ld=32,
                work=None)
    check_rejections(_lib.load().pss_harmonic_search, good,
                    ((dict(spec=None, work=p), "spec"), (dict(nl=0, work=p), "nl 0"), (dict(ndm=0, work=p), "ndm 0"),(dict(spec=None), "spec"), (dict(scale=None), "scale"), (dict(snr=None), "snr"),
                     (dict(code=None), "code"),
                     (dict(ndm=0), "ndm 0"), (dict(ndm=-2), "ndm -2"),
                     (dict(nbin=0), "nbin 0"), (dict(nbin=-1, ld=0), "nbin -1"),
                     (dict(nbin=(1 << 27) + 1, ld=1 << 28, out_ld=1 << 27), "2^27"),
                     (dict(ld=999), "ld 999"),
                     (dict(nl=0), "nl 0"), (dict(nl=6), "nl 6"), (dict(nl=-1), "nl -1"),
                     (dict(kmin=0), "kmin 0"), (dict(kmin=-3), "kmin -3"),
                     (dict(cell=8), "cell 8"), (dict(cell=0), "cell 0"), (dict(cell=48), "cell 48"),
                     (dict(cell=4096), "cell 4096"), (dict(cell=-32), "cell -32"),
                     (dict(out_ld=31), "out_ld 31"), (dict(cell=16, out_ld=62), "out_ld 62"),
                     (dict(nbin=1025, ld=1025, out_ld=32), "out_ld 32"),
                     # the launch grid: ceil(nbin / 2048) * ndm workgroups in 31 bits
                     (dict(nbin=1 << 27, ld=1 << 27, out_ld=1 << 27, ndm=1 << 16), "workgroups")),
                     prefix="harmonic_search")


def test_wiring():
    from psrsigsim_amd import build, telescope
    assert "pss_harmsum.hip" in build.UNITS
    assert any(d.endswith("pss_harmsum.hip") for d in build.DEPS)
    assert "pss_harmonic_search" in _lib.EXPORTS and hasattr(_lib.load(), "pss_harmonic_search")
    for name in ("HarmonicPlane", "PeriodCandidates", "DedispersedPlane", "Backend"):
        assert hasattr(telescope, name)
    for name in ("fft_length", "dm_spectrum", "harmonic_snr", "periodicity_search", "_harmonic_plan"):
        assert hasattr(telescope.Backend, name)


# ---------------------------------------------------------------------------
# the restatement itself
# ---------------------------------------------------------------------------
def test_restatement_on_a_hand_computed_row():
    """|X|^2 = 0 1 4 9 0 25 1 16 (k = 0 .. 7), scale 1, three levels, two
    "cells" of 4 (the restatement takes any cell; the kernel's start at 16):
      idx(k,1,2) = (k+1)/2 = 0 1 1 2 2 3 3 4      H_1 = P + P[idx] = 0  2  5 13  4 34 10 16
      idx(k,1,4) = (k+2)/4 = 0 0 1 1 1 1 2 2      idx(k,3,4) = (3k+2)/4 = 0 1 2 2 3 4 5 5
      H_2 = H_1 + P[idx(.,1,4)] + P[idx(.,3,4)]  = 0  3 10 18 14 35 39 45
      z_0 = P - 1, z_1 = (H_1 - 2) r, z_2 = (H_2 - 4) / 2, r = fp32(sqrt 2) / 2
    with kmin = 1 the fundamental's bin idx(k,1,h) must be >= 1: k >= 1 at every level."""
    X = np.array([[0, 1, 2j, 3, 0, 3 + 4j, -1j, -4]], dtype=np.complex64)
    r = np.float32(ref.SQRT2_F32 * np.float32(0.5))
    assert ref.coef(0) == 1.0 and ref.coef(1) == r and ref.coef(2) == 0.5 and ref.coef(3) == np.float32(r * 0.5)
    assert ref.coef(4) == 0.25
    assert np.array_equal(ref.power(X[0], 1.0), [0, 1, 4, 9, 0, 25, 1, 16])
    bz, bl = ref.best_per_bin(X[0], 1.0, 3, 1)
    z0 = np.array([-1, 0, 3, 8, -1, 24, 0, 15], dtype=np.float32)
    z1 = (np.array([0, 2, 5, 13, 4, 34, 10, 16], dtype=np.float32) - np.float32(2)) * r
    z2 = (np.array([0, 3, 10, 18, 14, 35, 39, 45], dtype=np.float32) - np.float32(4)) * np.float32(0.5)
    want = np.maximum(np.maximum(z0, z1), z2)
    want[0] = -np.inf                                      # k = 0: the fundamental is bin 0 < kmin
    assert np.array_equal(bz, want)
    #   z_0 = -1    0     3     8    -1    24     0    15
    #   z_1 = -1.41 0     2.12  7.78  1.41 22.6   5.66  9.90
    #   z_2 = -2   -0.5   3     7     5    15.5  17.5  20.5
    # k = 1 and k = 2 are ties (0 = 0, 3 = 3): the lower level
    assert np.array_equal(bl, [0, 0, 0, 0, 2, 0, 2, 2])
    snr, code = ref.harmonic_ref(X, 1.0, 3, 1, 4)
    assert snr.dtype == np.float32 and code.dtype == np.int32
    assert np.array_equal(snr, [[8.0, 24.0]])
    assert np.array_equal(code, [[(0 << 16) | 3, (0 << 16) | 1]])
    k, lev = ref.decode(code, 4)
    assert np.array_equal(k, [[3, 5]]) and np.array_equal(lev, [[0, 0]])
    # without bin 5 the second cell goes to k = 7 alone: z_0 = 15 (its z_2 is (16 + 0 + 4 + 0 - 4) / 2 = 8)
    X5 = np.array(X)
    X5[0, 5] = 0
    snr, code = ref.harmonic_ref(X5, 1.0, 3, 1, 4)
    assert np.array_equal(snr, [[8.0, 15.0]]) and np.array_equal(code, [[3, 3]])
    # P[6] = 16, P[7] = 9: at k = 6 z_0 = 15 and z_1 = (16 + P[3] - 2) r = 23 r = 16.3 -- two harmonics win
    X5[0, 7] = 3
    X5[0, 6] = 4
    snr, code = ref.harmonic_ref(X5, 1.0, 3, 1, 4)
    assert np.array_equal(snr, [[8.0, np.float32(23) * r]]) and np.array_equal(code, [[3, (1 << 16) | 2]])
    assert np.array_equal(ref.decode(code, 4)[0], [[3, 6]]) and np.array_equal(ref.decode(code, 4)[1], [[0, 1]])
    # the scale enters the power: half the amplitude, four times the scale, the same bits
    snr2, code2 = ref.harmonic_ref(X5 * np.float32(0.5), 4.0, 3, 1, 4)
    assert np.array_equal(snr2, snr) and np.array_equal(code2, code)
    # kmin = 2: level l is valid from k = 2 2^l - 2^(l-1): 2, 3, 6
    bz, bl = ref.best_per_bin(X[0], 1.0, 3, 2)
    assert np.array_equal(np.isfinite(bz), [False, False, True, True, True, True, True, True])
    assert bl[2] == 0 and bz[2] == 3.0 and bl[3] == 0 and bz[3] == 8.0          # (level 2's tie at k = 2 is gone)
    assert bl[4] == 1 and bz[4] == np.float32(2) * r                             # level 2 (z = 5) is not valid at k = 4
    # ties go to the lower level, then the lower bin; a NaN never wins; an all-NaN cell gives -inf, 0
    Y = np.array([[1, 1, 1, 1, np.nan, np.nan, np.nan, np.nan, 1, 1, np.nan, 1]], dtype=np.complex64)
    snr, code = ref.harmonic_ref(Y, 1.0, 2, 1, 4)
    assert np.array_equal(snr, np.array([[0.0, -np.inf, 0.0]], dtype=np.float32))
    assert np.array_equal(code, [[1, 0, 0]])
    # the normalisation
    s = ref.scale_f32([4.0, 0.0, -1.0, np.nan, np.inf], 100)
    assert s.dtype == np.float32 and np.array_equal(s, np.array([0.0025, 0, 0, 0, 0], dtype=np.float32))


# ---------------------------------------------------------------------------
# clustering and candidates
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dm_tol", [0, 1, 2])
@pytest.mark.parametrize("freq_tol", [0.0625, 1.0, 3.0])
def test_candidates_equal_all_pairs(dm_tol, freq_tol):
    from psrsigsim_amd.telescope.backend import period_candidates_from_cells, PERIOD_DTYPE
    rng = np.random.default_rng(2000 + 10 * dm_tol + int(16 * freq_tol))
    n = 1500
    j = rng.integers(0, 30, size=n)
    lev = rng.integers(0, 5, size=n)
    # fundamentals, with their fractions of a bin, over a range that grows with the tolerance, so that
    # neither partition is trivial
    k = (rng.integers(1, int(640 * freq_tol), size=n) << lev) + rng.integers(0, 1 << lev)
    snr = rng.integers(20, 60, size=n).astype(np.float32) / 2          # many equal values: the tie-breaks matter
    df = 0.125
    cand = period_candidates_from_cells(snr, j, k, lev, np.arange(30) * 2.5, df, dm_tol, freq_tol)
    expect = ref.candidates_ref(snr, j, k, lev, dm_tol, freq_tol)
    assert cand.dtype == PERIOD_DTYPE
    assert 20 < len(expect) < n - 20, len(expect)
    got = [(float(c["snr"]), int(c["dm_index"]), int(c["bin"]), int(c["nharm"]), int(c["ncells"])) for c in cand]
    assert got == expect
    assert int(cand["ncells"].sum()) == n
    assert np.array_equal(cand["dm"], 2.5 * cand["dm_index"])
    assert np.array_equal(cand["freq"], cand["bin"] / cand["nharm"].astype(np.float64) * df)
    assert np.array_equal(cand["period"], 1.0 / cand["freq"])


def test_friend_rule_levels_and_order():
    from psrsigsim_amd.telescope.backend import period_candidates_from_cells
    dms = np.arange(6) * 10.0
    # one fundamental of 100 bins seen at level 0 (k = 100), level 2 (k = 400) and level 4 (k = 1601:
    # 100.0625 bins), a neighbour a whole bin up at level 1 (k = 202), its second harmonic alone (k = 200
    # at level 0), and the same fundamental three trials away
    j = np.array([2, 2, 2, 2, 2, 5])
    k = np.array([100, 400, 1601, 202, 200, 100])
    lev = np.array([0, 2, 4, 1, 0, 0])
    snr = np.array([12, 14, 14, 11, 30, 13], dtype=np.float32)
    c = period_candidates_from_cells(snr, j, k, lev, dms, 0.5, dm_tol=1, freq_tol=0.0625)
    # at a sixteenth: {100, 400/4, 1601/16} join, 202/2 = 101 stays apart, 200 is another frequency
    assert c["snr"].tolist() == [30.0, 14.0, 13.0, 11.0]
    assert c["bin"].tolist() == [200, 400, 100, 202] and c["nharm"].tolist() == [1, 4, 1, 2]
    assert c["ncells"].tolist() == [1, 3, 1, 1] and c["dm_index"].tolist() == [2, 2, 5, 2]
    assert c["freq"].tolist() == [100.0, 50.0, 50.0, 50.5] and c["period"].tolist() == [0.01, 0.02, 0.02, 1 / 50.5]
    # equal snr inside a cluster: the lower bin (here the fewer harmonics) is the candidate
    c0 = period_candidates_from_cells(snr, j, k, lev, dms, 0.5, dm_tol=1, freq_tol=0.0)
    assert c0["ncells"].tolist() == [1, 2, 1, 1, 1] and c0["bin"].tolist() == [200, 400, 1601, 100, 202]
    # a whole bin of tolerance joins 101 too; three trials away stays apart until dm_tol 3
    c1 = period_candidates_from_cells(snr, j, k, lev, dms, 0.5, dm_tol=1, freq_tol=1.0)
    assert c1["ncells"].tolist() == [1, 4, 1] and c1["bin"].tolist() == [200, 400, 100]
    c3 = period_candidates_from_cells(snr, j, k, lev, dms, 0.5, dm_tol=3, freq_tol=1.0)
    assert c3["ncells"].tolist() == [1, 5] and c3["dm_index"].tolist() == [2, 2]
    # equal snr across candidates: (dm_index, bin, nharm) ascending
    c = period_candidates_from_cells(np.full(4, 20.0, dtype=np.float32), [3, 1, 1, 1], [64, 640, 64, 128],
                                     [0, 0, 0, 1], dms, 1.0, dm_tol=0, freq_tol=0.0)
    assert c["dm_index"].tolist() == [1, 1, 3] and c["bin"].tolist() == [64, 640, 64] and c["ncells"].tolist() == [2, 1, 1]
    e = period_candidates_from_cells(np.zeros(0, dtype=np.float32), [], [], [], dms, 0.5)
    assert len(e) == 0


def test_log_fap():
    """One harmonic: P(exp(1) >= snr + 1) = e^-(snr + 1).  h harmonics: the
    Erlang tail e^-H sum_{i < h} H^i / i! at H = snr sqrt(h) + h."""
    from math import factorial
    from psrsigsim_amd.telescope.backend import harmonic_log_fap, period_candidates_from_cells
    s = np.array([0.0, 1.0, 10.0, 15.0, 47.8])
    assert np.allclose(harmonic_log_fap(s, 1), -(s + 1), rtol=1e-12, atol=0)
    for h in (2, 4, 16):
        H = s * np.sqrt(h) + h
        want = -H + np.log(sum(H ** i / factorial(i) for i in range(h)))
        assert np.allclose(harmonic_log_fap(s, h), want, rtol=1e-10, atol=0)
    c = period_candidates_from_cells(np.array([10.0], dtype=np.float32), [0], [7], [0], [0.0], 1.0)
    assert c["log_fap"][0] == pytest.approx(-11.0, rel=1e-12)
    c = period_candidates_from_cells(np.array([10.0], dtype=np.float32), [0], [64], [4], [0.0], 1.0)
    assert -40 < c["log_fap"][0] < -20 and c["nharm"][0] == 16             # nowhere near a Gaussian's -53


def test_period_candidates_container():
    from psrsigsim_amd.telescope import PeriodCandidates
    from psrsigsim_amd.telescope.backend import period_candidates_from_cells
    arr = period_candidates_from_cells(np.array([18, 17], dtype=np.float32), [2, 5], [10, 900], [0, 2],
                                       np.arange(6) * 5.0, 0.01)
    pc = PeriodCandidates(arr, "cells", 15.0)
    assert len(pc) == 2 and pc.cells == "cells" and pc.threshold == 15.0
    assert pc.snr.tolist() == [18.0, 17.0] and pc.dm.tolist() == [10.0, 25.0] and pc.nharm.tolist() == [1, 4]
    assert pc[1]["bin"] == 900 and pc.array is arr and pc.freq.tolist() == [0.1, 2.25]
    with pytest.raises(AttributeError):
        pc.nothing


def test_max_cells_names_the_threshold(monkeypatch):
    """More cells above the threshold than max_cells: a ValueError that names
    the threshold (harmonic_snr stubbed: no device)."""
    import torch
    from psrsigsim_amd.telescope import Backend, HarmonicPlane
    pl = _plane(ndm=2, T=128)
    snr = torch.tensor([[17.0, 3.0], [18.0, 19.0]])
    k = torch.tensor([[3, 40], [6, 33]])
    lev = torch.tensor([[0, 1], [1, 0]], dtype=torch.int32)
    cells = HarmonicPlane(snr, k, lev, None, None, 2.0, 128, 64, 1, 32, None, None, pl)
    monkeypatch.setattr(Backend, "harmonic_snr", lambda self, plane, **kw: cells)
    be = _backend()
    with pytest.raises(ValueError, match=r"3 cells at or above threshold 16 exceed max_cells 2"):
        be.periodicity_search(pl, threshold=16.0, max_cells=2)
    got = be.periodicity_search(pl, threshold=16.0, max_cells=3, dm_tol=0)
    assert got.cells is cells and len(got) == 3
    assert got.snr.tolist() == [19.0, 18.0, 17.0] and got.dm_index.tolist() == [1, 1, 0]
    assert got.bin.tolist() == [33, 6, 3] and got.nharm.tolist() == [1, 2, 1] and got.freq.tolist() == [66.0, 6.0, 6.0]
    # bins 3 (trial 0) and 6 / 2 (trial 1) are one fundamental: at dm_tol 1 they join
    assert len(be.periodicity_search(pl, threshold=16.0, dm_tol=1, freq_tol=0.0)) == 2
