"""The case scripts of tests/single_batched_cases.py on the host: what
tests/test_gpu_single_batched.py relies on before it runs them on the device
-- the lengths classify as intended, the rows-per-workgroup table follows
the kernel's rule, the oracle alone keeps every delayed null inside the
ambiguity cap, the seeds the resampled copies use leave no ambiguous sample,
and the resampling multipliers reach the intended branch."""
import numpy as np
import pytest

from oracle import pss_cpu as O
from tests import replay
from tests import single_batched_cases as C


def _every_case():
    return (C.chain_cases() + C.shard_cases() + [c[:3] for c in C.window_cases()] + C.direct_cases())


def _oracle(case, seed, _cache={}):
    key = (repr(case), seed)
    if key not in _cache:
        _cache[key] = replay.oracle_exec(case, O.LegacyDraws(seed))
    return _cache[key]


def test_batch_table_follows_the_kernel_s_rule():
    # BATCH N = 4096, one row at 8192: launch_single_n (csrc/pss_single.hip)
    # is the source of this rule -- its template arguments are the table
    assert sorted(C.BATCH) == [1 << m for m in range(6, 14)] == sorted(C.ALL_SINGLE)
    for N, B in C.BATCH.items():
        assert B * N == (8192 if N == 8192 else 4096), (N, B)
    assert [C.nchan_of(N) for N in C.LENGTHS] == [67, 35, 19, 11, 7, 5]
    for N in C.LENGTHS:
        B, n = C.BATCH[N], C.nchan_of(N)
        # two workgroups (three at BATCH = 2), the last partly filled, an odd count
        assert -(-n // B) == (3 if B == 2 else 2) and 0 < n % B < B and n % 2 == 1
        nfull, pair = C.shards(N)
        assert pair == ((1, B + 2), (B, B + 3)) and nfull > B + 3
        assert C.rowcounts(N) == sorted({1, B - 1, B, B + 1, 2 * B + 1})


def test_every_case_classifies_as_intended():
    from psrsigsim_amd import _lib
    seen = set()
    for tag, case, _ in _every_case():
        N = C.nsamp_of(case)
        delayed = case["ops"][-2][0] == "null"
        kind = _lib.plan_geometry(N, 1 if delayed else 0)
        want = ("single", 1, N) if N in C.BATCH else ("direct", 0, 0)
        assert kind == want, (tag, N, kind)
        seen.add((N, delayed))
    for N in C.LENGTHS + C.DIRECT:
        assert (N, True) in seen and (N, False) in seen, N
    # the exact window sums' third length is off both (its run is elementwise: no delay)
    assert _lib.plan_geometry(10006, 0)[0] == "bluestein"


def test_case_shapes_and_parameters():
    for tag, case, seed in _every_case():
        A, inj = _oracle(case, seed)
        N = C.nsamp_of(case)
        sg = case["sig"]
        rows = sg["chans"][1] - sg["chans"][0] if sg.get("chans") else sg["nchan"]
        last = [op[-1] for op in case["ops"] if op[-1] is not None and op[0] != "observe"][-1]
        assert A["data_" + last].shape == (rows, N), tag
        assert A["out"].shape[0] == rows, tag
        if N in C.BATCH:
            assert int((sg["samprate"] * C.PERIOD) * 1e6) == N // 8, tag          # Nph samples per period
        if "null_pulses" in inj:
            assert len(inj["null_pulses"]) == 2, tag                               # 2 of 8 pulses
        if case["ops"][-1][1] == "Arecibo":
            assert A["out"].shape == (rows, N), tag                                # the full-rate copy
    # the delays grow as N^2 (the DM and the sample rate both grow with N): 0.05 .. 0.09
    # samples at N = 64, 54 .. 94 at 2048.  Neighbouring rows differ by > 3.9e-4 samples
    # everywhere, about ten times what TOL resolves on these noise-like rows, so a row
    # that took its neighbour's ramp is seen at every length
    for N in C.LENGTHS:
        sig = O.Signal(1400, 400, nchan=C.nchan_of(N), samprate=C.samprate(N), fold=False)
        d = np.asarray(O.dm_delays_ms(sig, C.dm_of(N))) * 1e-3 / (C.PERIOD / (N // 8))
        assert 0.09 * (N / 64) ** 2 < d.max() < 0.1 * (N / 64) ** 2, (N, d.max())
        assert np.abs(np.diff(d)).min() > 3.9e-4, (N, np.abs(np.diff(d)).min())


def test_oracle_alone_stays_within_the_ambiguity_cap():
    cases = C.null_cases()
    assert len(cases) >= 12 + 3 + 9 + 4
    for tag, case, seed in cases:
        _, inj = _oracle(case, seed)
        amb = inj["ambiguous"]
        assert inj["ambig_path"] == "packed", tag
        frac = amb.sum() / amb.size
        assert frac <= replay.AMBIG_MAX_FRAC["packed"], (tag, frac)
        assert frac <= 4.5e-4, (tag, frac)                                         # (as measured; well inside)


def test_resampled_null_seeds_have_no_ambiguous_sample():
    n = 0
    for tag, case, seed, _ in C.window_cases():
        _, inj = _oracle(case, seed)
        if "ambiguous" in inj:
            assert seed == C.ZERO_AMBIG_SEED[C.nsamp_of(case)]
            assert int(inj["ambiguous"].sum()) == 0, tag
            n += 1
    assert n == len(C.WINDOW_LENGTHS) * len(C.MULTS) + len(C.ONE_WINDOW)


@pytest.mark.parametrize("fold", [False, True], ids=["search", "fold"])
def test_resample_multipliers_reach_their_branch(fold):
    for N, m in [(N, m) for N in C.LENGTHS for m in C.MULTS] + [(250, 2.3)] + sorted(C.ONE_WINDOW.items()):
        case = C.case(N, fold=fold, null=None, mult=m)
        sg = case["sig"]
        sig = O.Signal(sg["fcent"], sg["bw"], nchan=sg["nchan"], samprate=sg["samprate"], sublen=sg.get("sublen"),
                       fold=fold)
        psr = O.Pulsar(C.PERIOD, 1.0, profiles=O.GaussPortrait(0.5, 0.05, 1))
        O.make_pulses(sig, psr, case["ops"][0][1], O.LegacyDraws(1))
        kind, arg = O.observe_branch(sig, 1.0 / case["ops"][-1][1][1], samprate_scale=1.0)
        assert kind == C.BRANCH[m], (N, fold, m, kind)
        # down_sample's factor; rebin's new length (windows of m samples, ceil-edged)
        assert arg == m if C.BRANCH[m] == "down" else N / m - 1 < arg <= (N + 0.5) / m, (N, fold, m, arg)
    if not fold:
        for tag, case, seed, branch in C.window_cases() + [C.direct_cases()[-1] + ("rebin",)]:
            A, _ = _oracle(case, seed)
            N = C.nsamp_of(case)
            one = tag.startswith(("64-x64", "128-x128"))
            want = (1,) if one else ((N // 4,) if branch == "down" else range(N // 6 + 1, N // 2))
            assert A["out"].shape[1] in want, tag
        assert sum(t[0].startswith(("64-x64", "128-x128")) for t in C.window_cases()) == 4
