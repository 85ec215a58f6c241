"""Incoherent dedispersion over trial DMs on the GPU (``pss_dedisperse``,
``Backend.dedisperse``).

The oracle is the float64 double loop over (trial, channel) of slices written
here (``oracle``):

    out[j][t] = sum_c data[c][t + d(j, c)],  t < T = n - max_delay,
    d = clip(table, 0, max_delay).

Index tests use integer-valued float32 data (seeded integers 0..15): every
partial sum is then an exact float32 in any order (C * 15 < 2^24) and the
comparison is ``array_equal`` -- no tolerance, no excluded sample.  Every
kernel-level case gives the kernel views inside larger tensors (row strides
ld > n and out_ld > T) whose guard regions hold a sentinel: the input's is
2^20 (a read outside a row's [0, n) lands in a sum and breaks the equality),
the output's is checked untouched afterwards.

The kernel's tile (pss_dedisperse.hip): a workgroup owns TB = 2048 output times
of ND = 8 neighbouring trials; a channel whose delays differ by at most
SPREAD = 2044 samples among those 8 trials is staged once in LDS, a wider one
goes trial by trial.
"""
import numpy as np
import pytest

from tests import kernel_harness as kh
from tests.kernel_harness import engine_seed_restored  # noqa: F401 (autouse here)

pytestmark = pytest.mark.gpu

TB, ND, SPREAD = 2048, 8, 2044
IN_GUARD = float(1 << 20)
OUT_GUARD = -7.0
DMS13 = np.arange(0, 65, 5)


def physical_table(ndm):
    """The API's own table: 64 channels, 1200-1600 MHz, 10 kHz sampling, DM 0, 5, ..."""
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.telescope import Backend
    sig = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False)
    return Backend.dedisperse_delays(sig, 5.0 * np.arange(ndm))


def oracle(data, table, max_delay):
    data = np.asarray(data, dtype=np.float64)
    d = np.clip(np.asarray(table, dtype=np.int64), 0, max_delay)
    T = data.shape[1] - max_delay
    out = np.zeros((d.shape[0], T))
    for j in range(d.shape[0]):
        for c in range(d.shape[1]):
            out[j] += data[c, d[j, c]:d[j, c] + T]
    return out


def int_data(C, N, seed):
    return np.random.default_rng(seed).integers(0, 16, size=(C, N)).astype(np.float32)


def _case(name):
    """(data [C][N] float32, table [nDM][C], max_delay) of the issue's cases."""
    if name == "copy":                                   # 1: degenerate
        return int_data(1, 64, 1), np.zeros((1, 1), dtype=np.int32), 0
    if name == "odd":                                    # 2: odd sizes, ragged tail, table not monotone
        tab = np.random.default_rng(2).integers(0, 38, size=(5, 3)).astype(np.int32)
        tab[3, 1] = 37
        return int_data(3, 1000, 20), tab, 37
    if name == "physical":                               # 3: the API's own shape
        tab = physical_table(13)
        assert tab.max() == 749
        return int_data(64, 16384, 3), tab, 749
    if name == "growing":                                # 4: spread grows with the trial; T = 1096
        j, c = np.arange(33)[:, None], np.arange(256)[None, :]
        tab = (j * (255 - c) ** 2 * 3000 // (255 ** 2 * 32)).astype(np.int32)
        assert tab.max() == 3000
        # its 8-trial groups stay inside the staged window (7 * 3000 / 32 = 656 <= SPREAD): "wide" below
        assert max(np.ptp(tab[g:g + ND], axis=0).max() for g in range(0, 33, ND)) <= SPREAD
        return int_data(256, 4096, 4), tab, 3000
    if name == "channels":                               # 5: many channels
        tab = np.zeros((2, 4096), dtype=np.int32)
        tab[1] = np.random.default_rng(5).integers(0, 101, size=4096)
        return int_data(4096, 2048, 50), tab, 100
    if name == "ragged":                                 # 6: T = one time tile + 1; 17 = 2 trial groups + 1
        tab = physical_table(17)
        md = int(tab.max())
        return int_data(64, TB + 1 + md, 6), tab, md
    if name == "wide":
        # beyond the staged window: random delays in [0, 3500] -- a group's spread
        # exceeds SPREAD in most channels (trial by trial), while channel 2
        # (constant) and channel 4 (spread exactly SPREAD) stay staged; T = 2500
        # is two time tiles, 9 trials are a full group and a single one
        tab = np.random.default_rng(9).integers(0, 3501, size=(9, 7)).astype(np.int32)
        tab[:, 2] = 1234
        tab[:, 4] = 100 + (np.arange(9) % 2) * SPREAD
        tab[0, 5], tab[7, 5] = 0, SPREAD + 1                # one past the window
        sp = np.ptp(tab[:ND], axis=0)
        assert sp[2] == 0 and sp[4] == SPREAD and sp[5] > SPREAD and (sp > SPREAD).sum() >= 4
        return int_data(7, 6000, 9), tab, 3500
    if name == "runs12":
        # 4 time tiles x 3 trial groups = 12 workgroups: more than the 8 XCDs and
        # no multiple of 8, so the XCD run map's runs differ in length (the other
        # cases launch 1 .. 6 workgroups, or 16)
        tab = physical_table(17)
        md = int(tab.max())
        return int_data(64, 3 * TB + 5 + md, 12), tab, md
    raise KeyError(name)


@kh.once
def reference(name):
    """A case and its float64 oracle, computed once and shared (read-only)."""
    data, tab, md = _case(name)
    return data, tab, md, oracle(data, tab, md)


def run_kernel(hip_lib, data, table, max_delay, ld=None, out_ld=None, in_off=0, out_off=0):
    """pss_dedisperse on views inside larger tensors (tests/kernel_harness.py):
    ``data`` with row stride ld between guards, ``out`` with row stride out_ld.
    Returns out [nDM][T] after checking that nothing outside out[j][0 .. T)
    was written."""
    import torch
    from psrsigsim_amd import _lib
    C, N = data.shape
    ndm = table.shape[0]
    T = N - max_delay
    ld = N + 5 if ld is None else ld
    out_ld = T + 3 if out_ld is None else out_ld
    assert ld > N and out_ld > T
    x = kh.GuardedInput(data, ld, in_off, IN_GUARD)
    out = kh.GuardedOutput(ndm, T, out_ld, out_off, OUT_GUARD)
    tab = torch.from_numpy(np.array(table, dtype=np.int32)).cuda()
    rc = hip_lib.pss_dedisperse(x.ptr, C, N, ld, tab.data_ptr(), ndm, max_delay, out.ptr, out_ld, None)
    _lib.check(rc, "dedisperse")
    torch.cuda.synchronize()
    return out.read()


KERNEL_CASES = ["copy", "odd", "physical", "growing", "channels", "ragged", "wide", "runs12"]


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_index_cases_equal_the_oracle(name, hip_lib):
    data, tab, md, ref = reference(name)
    N, T = data.shape[1], data.shape[1] - md
    if name == "ragged":
        assert T == TB + 1
    # rows on the 16-B grid (16-B loads of the windows) with an odd out_ld
    ld = (N + 3) // 4 * 4 + 4
    got = run_kernel(hip_lib, data, tab, md, ld=ld, out_ld=T + 1 + (T % 2))
    assert got.shape == ref.shape == (tab.shape[0], T)
    assert np.array_equal(got.astype(np.float64), ref)


@pytest.mark.parametrize("name", ["odd", "wide", "ragged"])
def test_misaligned_views_give_the_same_bits(name, hip_lib):
    """data base off by one float and an odd ld (element loads), out off by one
    float and an odd out_ld: bitwise equal to the aligned run, path by path."""
    data, tab, md, ref = reference(name)
    N, T = data.shape[1], data.shape[1] - md
    Na, Ta = (N + 3) // 4 * 4, (T + 3) // 4 * 4
    base = run_kernel(hip_lib, data, tab, md, ld=Na + 4, out_ld=Ta + 4)
    assert np.array_equal(base.astype(np.float64), ref)
    for kw in kh.misaligned_layouts(Na + 4, Ta + 4, kh.odd(N + 2), kh.odd(T + 2)):
        got = run_kernel(hip_lib, data, tab, md, **kw)
        assert got.tobytes() == base.tobytes(), kw


def test_clamp(hip_lib):
    """Entries below 0 and above max_delay are clamped as the table is loaded:
    the oracle of the clipped table, and no read outside a row's [0, n) (the
    guards around the rows would land in a sum)."""
    data, tab0, md, _ = reference("odd")
    tab = np.array(tab0)
    tab[0, 0] = -1
    tab[2, 1] = md + 1
    tab[4, 2] = -(1 << 31)
    tab[1, 2] = (1 << 31) - 1
    tab[3, 0] = md + 4096
    ref = oracle(data, np.clip(tab.astype(np.int64), 0, md), md)
    got = run_kernel(hip_lib, data, tab, md)
    assert np.array_equal(got.astype(np.float64), ref)
    # the same in the trial-by-trial path
    data, tab0, md, _ = reference("wide")
    tab = np.array(tab0)
    tab[1, 0], tab[6, 0], tab[3, 3], tab[8, 6] = -5, md + 1, (1 << 31) - 1, -(1 << 31)
    ref = oracle(data, np.clip(tab.astype(np.int64), 0, md), md)
    got = run_kernel(hip_lib, data, tab, md)
    assert np.array_equal(got.astype(np.float64), ref)


def test_float_data_within_the_any_order_bound(hip_lib):
    """chi2(1) draws plus one sample of 1e4 per channel, case 3's shape: every
    output within gamma * sum_c |x|, gamma = (C-1)u / (1 - (C-1)u), u = 2^-24
    (the bound of a float32 sum of C terms in any order; derived, not
    measured); two launches give the same bits."""
    _, tab, md, _ = reference("physical")
    C, N = 64, 16384
    rng = np.random.default_rng(31)
    x = rng.chisquare(1, size=(C, N))
    x[np.arange(C), rng.integers(0, N, size=C)] = 1e4
    x = x.astype(np.float32)
    ref = oracle(x, tab, md)
    mag = oracle(np.abs(x), tab, md)
    u = 2.0 ** -24
    gamma = (C - 1) * u / (1 - (C - 1) * u)
    got = run_kernel(hip_lib, x, tab, md, ld=N + 4, out_ld=N - md + 4)
    err = np.abs(got.astype(np.float64) - ref)
    print("float test: max err / bound", float((err / (gamma * mag)).max()))
    assert (err <= gamma * mag).all()
    again = run_kernel(hip_lib, x, tab, md, ld=N + 4, out_ld=N - md + 4)
    assert again.tobytes() == got.tobytes()


# ---------------------------------------------------------------------------
# API
# ---------------------------------------------------------------------------
def test_api_on_a_search_mode_signal(hip_lib):
    import torch
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.telescope import DedispersedPlane
    data, tab, md, ref = reference("physical")
    sig = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False)
    sig._buf = torch.from_numpy(np.array(data)).cuda()
    sig._ncols = sig._nsamp = data.shape[1]
    plane = kh.backend().dedisperse(sig, DMS13)
    assert isinstance(plane, DedispersedPlane)
    T = data.shape[1] - md
    assert tuple(plane.data.shape) == (13, T) and plane.data.dtype == torch.float32 and plane.data.is_cuda
    assert plane.data.stride(0) % 4 == 0 and plane.data.stride(1) == 1 and plane.data.data_ptr() % 16 == 0
    assert np.array_equal(plane.data.cpu().numpy().astype(np.float64), ref)
    assert plane.dms.dtype == np.float64 and np.array_equal(plane.dms, DMS13)
    assert plane.delays.dtype == np.int32 and np.array_equal(plane.delays, tab)
    assert plane.max_delay == md == 749 and plane.ref_freq == 1593.75 and plane.samprate == 0.01
    assert sig.data.cpu().numpy().tobytes() == data.tobytes()           # the signal is left as it was
    # a sharded signal: this rank's partial sum over its channels, common reference
    part = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False, shard=(16, 48))
    part._buf = torch.from_numpy(np.array(data[16:48])).cuda()
    part._ncols = part._nsamp = data.shape[1]
    pp = kh.backend().dedisperse(part, DMS13)
    assert np.array_equal(pp.delays, tab[:, 16:48])
    mdp = int(tab[:, 16:48].max())
    assert np.array_equal(pp.data.cpu().numpy().astype(np.float64), oracle(data[16:48], tab[:, 16:48], mdp))


def test_api_accepts_the_channelised_signal(hip_lib):
    import torch
    from psrsigsim_amd.signal import BasebandSignal
    be = kh.backend()
    bb = BasebandSignal(1400, 0.512, Nchan=2)
    n = 32 * 300 + 7
    g = torch.Generator(device="cuda").manual_seed(7)
    bb._buf = torch.randn((2, n), dtype=torch.float32, device="cuda", generator=g)
    bb._ncols = bb._nsamp = n
    fb = be.channelize(bb, 16)
    S = 300
    assert tuple(fb.data.shape) == (16, S)
    dms = np.array([0.0, 100.0, 300.0, 700.0])    # 31.25 us samples over 1399.744-1400.224 MHz: up to ~33 samples
    plane = be.dedisperse(fb, dms)
    md = plane.max_delay
    assert md == int(plane.delays.max()) and 0 < md < S
    assert tuple(plane.data.shape) == (4, S - md)
    x = fb.data.cpu().numpy()
    ref = oracle(x, plane.delays, md)
    mag = oracle(np.abs(x), plane.delays, md)
    u = 2.0 ** -24
    gamma = 15 * u / (1 - 15 * u)
    assert (np.abs(plane.data.cpu().numpy().astype(np.float64) - ref) <= gamma * mag).all()


def test_injected_dm_is_recovered(hip_lib):
    """make_pulses -> ISM.disperse(30) -> dedisperse(0, 5, .. 60): the variance
    over time of the trial series peaks at DM 30, at least 1.15 x the runner-up
    (the CPU oracle gives 1.29-1.30 over 12 seeds; the device draws from another
    generator, and 1.15 leaves ten times that seed-to-seed spread)."""
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar
    from psrsigsim_amd.ism import ISM
    pss.seed(20250101)
    sig = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False)
    psr = Pulsar(0.05, 1.0)
    psr.make_pulses(sig, tobs=1.6384)
    ISM().disperse(sig, 30)
    assert tuple(sig.data.shape) == (64, 16384)
    plane = kh.backend().dedisperse(sig, DMS13)
    assert tuple(plane.data.shape) == (13, 16384 - 749)
    var = plane.data.double().var(dim=1).cpu().numpy()
    order = np.argsort(var)
    print("variance per trial", var, "ratio", var[order[-1]] / var[order[-2]])
    assert int(np.argmax(var)) == 6
    assert var[order[-1]] >= 1.15 * var[order[-2]]
