"""The fused run on the lengths the single-workgroup kernel serves with
several rows per workgroup (csrc/pss_single.hip: N = 64 .. 2048, BATCH = 64 ..
2 rows) and on the direct DFT, with a real source and every epilogue feature.

The cases are tests/single_batched_cases.py's: BATCH + 3 channels (two
workgroups, the last partly filled), eight periods, a delay of a few to tens
of samples across the band.

(a) the whole chain -- source, delay ramp, delayed or undelayed null,
    observe's full-rate copy (float32 / int8), noise -- against the float64
    oracle with injected draws, fused and staged (the staged delayed null is
    the mask-only run that loads its data in the epilogue);
(b) shards of a wider band against the oracle, and with Philox draws against
    the same rows of the full-band run, bit for bit;
(c) with Philox draws, a row does not depend on how many rows run with it;
(d) observe's window sums (down_sample / rebin) where a wave holds four, two
    and one row(s): against the oracle, repeatable, the data untouched; and
    exact window sums of integer-valued samples on the elementwise path;
(e) the direct DFT (N = 32, 66, 250, 1000) with a delayed null (the float64
    refine over the direct rows) and without.

Tolerance: per channel max|gpu - ref| / max|ref| <= 1e-5 (BASELINE north_star)
and replay.py's null caps, unchanged.  Every run's launch plan is asserted.
"""
import numpy as np
import pytest

from oracle import pss_cpu as O
from tests import replay
from tests import single_batched_cases as C
from tests.kernel_harness import engine_seed_restored, same_bits  # noqa: F401 (autouse here)

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _plan_tokens(N):
    return ("single", str(N)) if N in C.BATCH else ("direct",)


def _assert_plan(lines, case, refine=False):
    """The last FFT run of the case's rows x N took the single-workgroup
    kernel of that length (or the direct DFT), and the float64 refine where a
    delayed null rides on it."""
    N = C.nsamp_of(case)
    ch = case["sig"].get("chans")
    rows = ch[1] - ch[0] if ch else case["sig"]["nchan"]
    tok = _plan_tokens(N)
    fft = [l for l in lines if tok[0] in l.split()]
    line = replay.assert_plan(fft, rows, N, tok, absent=("bluestein", "fourstep", "smooth"))
    if refine:
        assert any(t.startswith("N:refine") for t in line.split()), line
    return line


def _vs_oracle(case, seed, fused):
    from psrsigsim_amd import _lib
    _lib.plan_collect()
    errs = replay.run_case(None, fused=fused, case=case, seed=seed)
    delayed = case["ops"][-2][0] == "null"
    line = _assert_plan(_lib.plan_collect(), case, refine=delayed)
    print("%s %s: %s" % ("fused" if fused else "staged", line,
                         ", ".join("%s %.3g" % kv for kv in sorted(errs.items()))))
    want = {"out"} | ({"noise"} if case["ops"][-1][3] else set())
    if not fused:
        want |= {op[-1] for op in case["ops"] if op[-1] is not None}
    assert want <= set(errs), (want, errs)
    bad = {k: v for k, v in errs.items() if not v <= TOL}
    assert not bad, errs


# ---------------------------------------------------------------------------
# (a) the full chain against the oracle
# ---------------------------------------------------------------------------
_CHAIN = C.chain_cases()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "staged"])
@pytest.mark.parametrize("case,seed", [c[1:] for c in _CHAIN], ids=[c[0] for c in _CHAIN])
def test_chain_vs_oracle(case, seed, fused, hip_lib):
    _vs_oracle(case, seed, fused)


@pytest.mark.parametrize("N", [64, 2048, 32])
def test_search_mode_null_keeps_the_mask_out_of_the_data_s_transform(N, hip_lib):
    """A delayed null's mask (chi2(100) draws, ~130) in the imaginary part of
    a search-mode row's transform (chi2(1) draws x a profile <= 1) left the
    row with the mask's fp32 error: the fused chains above measured 1.3e-5
    (N = 128) .. 2.6e-5 (64) and 3.4e-4 (32, direct DFT) of the row's maximum,
    where the staged chains (the mask transformed alone) gave <= 1.5e-6.  The
    fused run now transforms the two apart, as the staged chain does: its plan
    notes the FFT twice, and its error is the staged chain's to within the
    noise stage's rounding.  A fold-mode row is as large as its mask and
    stays packed (one FFT)."""
    from psrsigsim_amd import _lib
    tok = _plan_tokens(N)[0]
    errs = {}
    for fused in (True, False):
        _lib.plan_collect()
        errs[fused] = replay.run_case(None, fused=fused, case=C.case(N), seed=1)
        if fused:
            line = _assert_plan(_lib.plan_collect(), C.case(N), refine=True)
            assert line.split().count(tok) == 2, line
    print("N=%d fused %s staged %s" % (N, errs[True], errs[False]))
    assert errs[True]["noise"] <= 2 * errs[False]["noise"] + 1e-7, errs
    if N in C.BATCH:
        _lib.plan_collect()
        replay.run_case(None, fused=True, case=C.case(N, fold=True), seed=2)
        line = _assert_plan(_lib.plan_collect(), C.case(N, fold=True), refine=True)
        assert line.split().count(tok) == 1, line


# ---------------------------------------------------------------------------
# Philox runs of a case script (no injection)
# ---------------------------------------------------------------------------
def _philox(case, seed=11, ret=True):
    """The case on the product with its own draws: (data, out or None, plan lines)."""
    import psrsigsim_amd as pss
    from psrsigsim_amd import _lib
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar, GaussProfile, DataProfile
    from psrsigsim_amd.ism import ISM
    from psrsigsim_amd.telescope import telescope as T
    from psrsigsim_amd.telescope import Telescope, Receiver, Backend
    from psrsigsim_amd._units import Quantity
    sg, ps = case["sig"], case["psr"]
    pss.seed(seed)
    _lib.plan_collect()
    sig = FilterBankSignal(sg["fcent"], sg["bw"], Nsubband=sg["nchan"], sample_rate=sg["samprate"],
                           sublen=sg.get("sublen"), dtype=sg["dtype"], fold=sg["fold"], shard=sg.get("chans"))
    spec = ps["prof"]
    prof = GaussProfile(*spec[1:]) if spec[0] == "gauss" else DataProfile(replay._prof(), Nchan=spec[1])
    psr = Pulsar(ps["period"], ps["Smean"], profiles=prof, specidx=ps.get("specidx", 0.0), ref_freq=ps.get("ref_freq"))
    out = None
    for op in case["ops"]:
        if op[0] == "make_pulses":
            psr.make_pulses(sig, op[1])
        elif op[0] == "disperse":
            ISM().disperse(sig, op[1])
        elif op[0] == "null":
            psr.null(sig, op[1])
        else:
            assert op[0] == "observe", op
            if op[1] == "Arecibo":
                tel = T.Arecibo()
            else:
                tel = Telescope(20.0, area=None, Tsys=25.0, name="Twenty_Meter")
                tel.add_system(name="T", receiver=Receiver(fcent=1400, bandwidth=400, name="Lband"),
                               backend=Backend(samprate=1.0 / Quantity(op[1][1], "s"), name="Cyborg"))
            out = tel.observe(sig, psr, system=op[2], noise=op[3], ret_resampsig=ret)
    data = sig.data.cpu().numpy()
    assert data.shape[1] == C.nsamp_of(case) and np.isfinite(data).all() and data.std() > 0
    return data, (out.cpu().numpy() if out is not None else None), _lib.plan_collect()


# ---------------------------------------------------------------------------
# (b) shards
# ---------------------------------------------------------------------------
_SHARD = C.shard_cases()


@pytest.mark.parametrize("case,seed", [c[1:] for c in _SHARD], ids=[c[0] for c in _SHARD])
def test_shard_vs_oracle(case, seed, hip_lib):
    _vs_oracle(case, seed, True)


@pytest.mark.parametrize("fold", [False, True], ids=["search", "fold"])
@pytest.mark.parametrize("N", C.LENGTHS)
def test_full_band_rows_match_shards(N, fold, hip_lib):
    """Philox draws are keyed by the global channel, the ramp and the profile
    table row are the global channel's: a shard's rows are the full band's."""
    nfull, pair = C.shards(N)
    kw = dict(fold=fold, null=None, nchan=nfull, prof=("data", nfull), specidx=-1.6)
    full_case = C.case(N, **kw)
    full, full_out, lines = _philox(full_case)
    _assert_plan(lines, full_case)
    assert full.shape == (nfull, N)
    assert len({row.tobytes() for row in full}) == nfull                  # no two rows alike
    for ch in pair:
        case = C.case(N, chans=ch, **kw)
        part, part_out, lines = _philox(case)
        _assert_plan(lines, case)
        assert same_bits(part, full[ch[0]:ch[1]]), (N, ch, np.argwhere(part != full[ch[0]:ch[1]])[:4])
        assert same_bits(part_out, full_out[ch[0]:ch[1]]), (N, ch)


# ---------------------------------------------------------------------------
# (c) a row does not depend on the row count
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", C.ROWCOUNT_LENGTHS)
def test_rows_do_not_depend_on_the_row_count(N, hip_lib):
    """Rows [0, n) of one band (2 BATCH + 1 channels), run alone for n = 1,
    BATCH - 1, BATCH, BATCH + 1 and 2 BATCH + 1 with noise and a delayed null:
    every row has the bits it has in the largest run (the batch a row falls
    in, its place in it and the partly filled last workgroup change nothing)."""
    B = C.BATCH[N]
    nfull = 2 * B + 1
    full_case = C.case(N, nchan=nfull)
    full, full_out, lines = _philox(full_case)
    _assert_plan(lines, full_case, refine=True)
    assert full.shape == (nfull, N) and len({row.tobytes() for row in full}) == nfull
    assert not np.array_equal(full, full_out)                             # (the copy is pre-noise)
    for n in C.rowcounts(N):
        if n == nfull:
            continue
        case = C.case(N, nchan=nfull, chans=(0, n))
        part, part_out, lines = _philox(case)
        _assert_plan(lines, case, refine=True)
        assert same_bits(part, full[:n]), (N, n, np.argwhere(part != full[:n])[:4])
        assert same_bits(part_out, full_out[:n]), (N, n)


# ---------------------------------------------------------------------------
# (d) window sums
# ---------------------------------------------------------------------------
_WINDOW = C.window_cases()


@pytest.mark.parametrize("case,seed,branch", [c[1:] for c in _WINDOW], ids=[c[0] for c in _WINDOW])
def test_window_sums_vs_oracle(case, seed, branch, hip_lib):
    """The resampled copy of a run whose waves hold 4 (N = 64), 2 (128) and 1
    (2048) rows against the oracle's down_sample / rebin; at 64 and 128 also
    down to ONE window per row, where alone neighbouring lanes of different
    rows hold the same window index.  With a delayed null
    the seed leaves no sample in the ambiguity band (asserted: the harness
    cannot exclude samples from a resampled copy)."""
    A, inj = replay.oracle_exec(case, O.LegacyDraws(seed))
    N, nchan = C.nsamp_of(case), case["sig"]["nchan"]
    assert A["out"].shape[0] == nchan and 1 <= A["out"].shape[1] < N // 2
    if "ambiguous" in inj:
        assert int(inj["ambiguous"].sum()) == 0
    _vs_oracle(case, seed, True)
    # Philox: two identical runs give the same bits, and the data are the plain run's
    a, a_out, lines = _philox(case)
    _assert_plan(lines, case, refine="ambiguous" in inj)
    b, b_out, _ = _philox(case)
    plain, none, _ = _philox(case, ret=False)
    assert none is None and a_out.shape == A["out"].shape, (a_out.shape, A["out"].shape)
    assert same_bits(a_out, b_out) and same_bits(a, b)
    assert same_bits(a, plain)


# (down_sample by f needs f | N: 10006 = 2 x 5003 takes f = 2)
_EXACT = [(N, nchan, m) for N, nchan, ms in ((64, 67, (4, 2.3, 5.5)), (128, 35, (4, 2.3, 5.5)), (10006, 3, (2, 2.3, 5.5)))
          for m in ms]


@pytest.mark.parametrize("N,nchan,mult", _EXACT, ids=["%d-x%g" % (n, m) for n, _, m in _EXACT])
def test_window_sums_exact_on_integer_samples(N, nchan, mult, hip_lib):
    """The elementwise run (no delay) of a constant profile with injected
    integer-valued draws: every sample is a small integer, so every window
    sum is exact in any order and the copy equals the oracle's down_sample /
    rebin of the data in bits -- a dropped or doubled piece, or a wrong
    window width, cannot hide under a tolerance."""
    import psrsigsim_amd as pss
    from psrsigsim_amd import _lib
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar, DataProfile
    from psrsigsim_amd.telescope import Telescope, Receiver, Backend
    from psrsigsim_amd._units import Quantity
    # the case builder's eight periods of N / 8 samples; 10006 samples at the default rate
    sr = C.samprate(N) if N in C.BATCH else None
    dt = 20.48e-6 if sr is None else 1.0 / (sr * 1e6)
    draws = np.random.default_rng(N).integers(0, 150, size=(nchan, N)).astype(np.float64)
    pss.seed(5)
    sig = FilterBankSignal(1400, 400, Nsubband=nchan, fold=False, sample_rate=sr)
    psr = Pulsar(C.PERIOD, 1.0, profiles=DataProfile(np.ones(64), Nchan=nchan))
    pss.inject(gen=draws)
    psr.make_pulses(sig, tobs=(N + 0.5) * dt)
    assert sig.nsamp == N
    dt_sig = float(getattr(sig.sublen, "value", sig.sublen)) / (sig.nsamp / sig.nsub)          # as observe() computes it
    tel = Telescope(20.0, area=None, Tsys=25.0, name="T")
    tel.add_system(name="S", receiver=Receiver(fcent=1400, bandwidth=400, name="L"),
                   backend=Backend(samprate=1.0 / Quantity(2 * mult * dt_sig, "s"), name="B"))
    kind = tel.resample_branch(sig, tel.systems["S"][1])
    assert kind[0] == ("down" if mult in (2, 4) else "rebin"), kind
    _lib.plan_collect()
    out = tel.observe(sig, psr, system="S", noise=False, ret_resampsig=True).cpu().numpy()
    replay.assert_plan(_lib.plan_collect(), nchan, N, ("elementwise",))
    data = sig.data.cpu().numpy()
    assert np.array_equal(data, draws)                                    # profile == 1 exactly
    res = O.down_sample if kind[0] == "down" else O.rebin
    ref = np.stack([res(row, kind[1]) for row in data.astype(np.float64)])
    ref = np.minimum(ref, float(sig._draw_max)).astype(np.float32)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert same_bits(out, ref), np.argwhere(out != ref)[:8]


# ---------------------------------------------------------------------------
# (e) the direct DFT
# ---------------------------------------------------------------------------
_DIRECT = C.direct_cases()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "staged"])
@pytest.mark.parametrize("case,seed", [c[1:] for c in _DIRECT], ids=[c[0] for c in _DIRECT])
def test_direct_dft_chain_vs_oracle(case, seed, fused, hip_lib):
    _vs_oracle(case, seed, fused)
