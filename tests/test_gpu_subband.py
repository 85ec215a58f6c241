"""Sub-band dedispersion on the GPU: the banded entry ``pss_dedisperse_banded``
and ``Backend.subband_dedisperse``.

The oracle is tests/subband_ref.py (float64 loops of slices).  Index tests use
integer-valued float32 data (seeded integers 0..15): every partial sum is then
an exact float32 in any order and the comparison is ``array_equal``.  The
kernel sees views inside larger tensors (tests/kernel_harness.py): the source
planes lie ``src_stride`` > nchan * ld apart with whole rows of the 2^20
sentinel between them, so a read outside a row's [0, n) or in another plane's
gap lands in a sum; the output's guards are checked untouched.

The tile (pss_dedisperse.hip): 2048 times x 8 trials of one source and one
band; a channel whose delays differ by at most 2044 samples among the 8 trials
is staged once, a wider one goes trial by trial.
"""
import numpy as np
import pytest

from tests import kernel_harness as kh
from tests import subband_ref as ref
from tests.kernel_harness import engine_seed_restored  # noqa: F401 (autouse here)

pytestmark = pytest.mark.gpu

TB, ND, SPREAD = 2048, 8, 2044
IN_GUARD = float(1 << 20)
OUT_GUARD = -7.0
GAP_ROWS = 2                                       # sentinel rows between two source planes


def physical_table(ndm):
    """The API's own table: 64 channels, 1200-1600 MHz, 10 kHz sampling, DM 0, 5, ..."""
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.telescope import Backend
    sig = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False)
    return Backend.dedisperse_delays(sig, 5.0 * np.arange(ndm))


def int_planes(nsrc, C, N, seed):
    return np.random.default_rng(seed).integers(0, 16, size=(nsrc, C, N)).astype(np.float32)


def float_planes(nsrc, C, N, seed):
    return np.random.default_rng(seed).random(size=(nsrc, C, N), dtype=np.float32) * 3 + 0.1


def wide_table():
    """7 channels, 9 trials, delays in [0, 3500]: channel 2 constant, channel 4 at spread 2044 (staged), channel 5 at
    2045 (trial by trial), the others random (mostly wide)."""
    tab = np.random.default_rng(9).integers(0, 3501, size=(9, 7)).astype(np.int32)
    tab[:, 2] = 1234
    tab[:, 4] = 100 + (np.arange(9) % 2) * SPREAD
    tab[0, 5], tab[7, 5] = 0, SPREAD + 1
    tab[1:7, 5] = np.clip(tab[1:7, 5], 0, SPREAD + 1)
    sp = np.ptp(tab[:ND], axis=0)
    assert sp[2] == 0 and sp[4] == SPREAD and sp[5] == SPREAD + 1
    return tab


def _case(name):
    """(planes [nsrc][C][N] float32, table [ndm][C], per_src, max_delay, band)."""
    if name == "direct_physical":                   # as direct: one source, one band, float data
        tab = physical_table(13)
        return float_planes(1, 64, 16384, 3), tab, 13, int(tab.max()), 64
    if name == "direct_wide":
        return float_planes(1, 7, 6000, 4), wide_table(), 9, 3500, 7
    if name == "direct_ragged":                     # T = one time tile + 1; 17 = 2 trial groups + 1
        tab = physical_table(17)
        md = int(tab.max())
        return float_planes(1, 64, TB + 1 + md, 6), tab, 1 << 30, md, 1 << 30
    if name == "bands":                             # bands of 8, 8, 6; 11 trials; T = 2049
        tab = np.random.default_rng(2).integers(0, 39, size=(11, 22)).astype(np.int32)
        tab[3, 1], tab[5, 20] = 38, 0
        return int_planes(1, 22, 2049 + 38, 20), tab, 11, 38, 8
    if name == "sources":                           # 13 trials of 3 sources: 5, 5, 3; one band of 6 channels
        tab = np.random.default_rng(5).integers(0, 61, size=(13, 6)).astype(np.int32)
        return int_planes(3, 6, 3000, 21), tab, 5, 60, 6
    if name == "both":
        # 2 sources x 9 trials (groups of 8 + 1 each), bands of 4, 4, 2; channel 5's delays spread by more than
        # SPREAD inside source 0's first 8 trials, beside staged channels of the same band: both paths in one workgroup
        tab = np.random.default_rng(7).integers(0, 301, size=(18, 10)).astype(np.int32)
        tab[2, 5], tab[6, 5] = 3, 3 + SPREAD + 1
        tab[11, 9], tab[12, 9] = 0, 3400
        assert np.ptp(tab[:8, 5]) > SPREAD and np.ptp(tab[:8, 4]) <= SPREAD and np.ptp(tab[9:17, 9]) > SPREAD
        return int_planes(2, 10, 6000, 22), tab, 9, 3400, 4
    if name == "runs27":
        # 3 time tiles x 3 bands x 3 trial groups = 27 workgroups: more than the 8 XCDs and no multiple of 8
        tab = np.random.default_rng(11).integers(0, 50, size=(13, 9)).astype(np.int32)
        return int_planes(3, 9, 2 * TB + 9 + 49, 23), tab, 5, 49, 3
    raise KeyError(name)


@kh.once
def reference(name):
    """A case and its float64 oracle [ndm][nb][T], computed once and shared (read-only)."""
    planes, tab, per_src, md, band = _case(name)
    return planes, tab, per_src, md, band, ref.banded(planes, tab, min(per_src, 1 << 20), md, min(band, 1 << 20))


def run_banded(hip_lib, planes, table, per_src, max_delay, band, ld=None, out_ld=None, in_off=0, out_off=0,
               stride_extra=0):
    """pss_dedisperse_banded on views inside larger tensors: the planes with row stride ld, GAP_ROWS sentinel rows
    (+ ``stride_extra`` floats) between them; ``out`` [ndm * nb][out_ld].  Returns out [ndm][nb][T] after checking
    that nothing outside the T samples of every row was written."""
    import torch
    from psrsigsim_amd import _lib
    nsrc, C, N = planes.shape
    ndm = table.shape[0]
    nb = -(-C // min(band, C))
    T = N - max_delay
    ld = N + 5 if ld is None else ld
    out_ld = T + 3 if out_ld is None else out_ld
    assert ld > N and out_ld > T
    # one guarded tensor of rows: every plane's C rows, then GAP_ROWS rows of sentinel; stride_extra sentinel floats
    # more per plane are had by viewing the rows at a stride (the kernel's src_stride), the rows' own words kept
    rows_per = C + GAP_ROWS
    src_stride = rows_per * ld + stride_extra
    flat = np.full(nsrc * src_stride, IN_GUARD, dtype=np.float32)
    for q in range(nsrc):
        for c in range(C):
            o = q * src_stride + c * ld
            flat[o:o + N] = planes[q, c]
    x = kh.GuardedInput(flat[None, :], flat.size, in_off, IN_GUARD)
    out = kh.GuardedOutput(ndm * nb, T, out_ld, out_off, OUT_GUARD)
    tab = torch.from_numpy(np.array(table, dtype=np.int32)).cuda()
    rc = hip_lib.pss_dedisperse_banded(x.ptr, nsrc, src_stride, C, N, ld, tab.data_ptr(), ndm, per_src, max_delay,
                                       band, out.ptr, out_ld, None)
    _lib.check(rc, "dedisperse_banded")
    torch.cuda.synchronize()
    return out.read().reshape(ndm, nb, T)


def run_direct(hip_lib, data, table, max_delay):
    import torch
    from psrsigsim_amd import _lib
    C, N = data.shape
    T = N - max_delay
    x = kh.GuardedInput(data, N + 4, 0, IN_GUARD)
    out = kh.GuardedOutput(table.shape[0], T, T + 3, 0, OUT_GUARD)
    tab = torch.from_numpy(np.array(table, dtype=np.int32)).cuda()
    _lib.check(hip_lib.pss_dedisperse(x.ptr, C, N, N + 4, tab.data_ptr(), table.shape[0], max_delay, out.ptr, T + 3,
                                      None), "dedisperse")
    torch.cuda.synchronize()
    return out.read()


@pytest.mark.parametrize("name", ["direct_physical", "direct_wide", "direct_ragged"])
def test_one_source_and_one_band_give_the_direct_kernels_bits(name, hip_lib):
    planes, tab, per_src, md, band, want = reference(name)
    N = planes.shape[2]
    got = run_banded(hip_lib, planes, tab, per_src, md, band, ld=(N + 3) // 4 * 4 + 4)
    assert got.shape == (tab.shape[0], 1, N - md)
    direct = run_direct(hip_lib, planes[0], tab, md)
    assert kh.same_bits(got[:, 0], direct)
    # (and both are the sum: float data, any order of C terms)
    mag = ref.banded(np.abs(planes), tab, 1 << 20, md, 1 << 20)
    assert (np.abs(got.astype(np.float64) - want) <= planes.shape[1] * 2.0 ** -24 * mag).all()
    # off the 16-B grid: the element loads give the same bits
    again = run_banded(hip_lib, planes, tab, per_src, md, band, ld=kh.odd(N + 2), in_off=1)
    assert kh.same_bits(again, got)


@pytest.mark.parametrize("name", ["bands", "sources", "both", "runs27"])
def test_index_cases_equal_the_oracle(name, hip_lib):
    planes, tab, per_src, md, band, want = reference(name)
    N = planes.shape[2]
    T = N - md
    if name == "bands":
        assert T == TB + 1 and want.shape[1] == 3
    if name == "runs27":
        assert -(-T // TB) * want.shape[1] * 3 == 27
    got = run_banded(hip_lib, planes, tab, per_src, md, band, ld=(N + 3) // 4 * 4 + 4, out_ld=T + 1 + (T % 2))
    assert got.shape == want.shape
    assert np.array_equal(got.astype(np.float64), want)


@pytest.mark.parametrize("name", ["bands", "both"])
def test_misaligned_layouts_give_the_same_bits(name, hip_lib):
    """data one float off the 16-B grid, an odd ld, an odd src_stride, an odd out_ld: the aligned run's bits, the
    guards untouched; and two runs give the same bits."""
    planes, tab, per_src, md, band, want = reference(name)
    N, T = planes.shape[2], planes.shape[2] - md
    Na, Ta = (N + 3) // 4 * 4, (T + 3) // 4 * 4
    base = run_banded(hip_lib, planes, tab, per_src, md, band, ld=Na + 4, out_ld=Ta + 4)
    assert np.array_equal(base.astype(np.float64), want)
    again = run_banded(hip_lib, planes, tab, per_src, md, band, ld=Na + 4, out_ld=Ta + 4)
    assert again.tobytes() == base.tobytes()
    for kw in kh.misaligned_layouts(Na + 4, Ta + 4, kh.odd(N + 2), kh.odd(T + 2)):
        got = run_banded(hip_lib, planes, tab, per_src, md, band, **kw)
        assert got.tobytes() == base.tobytes(), kw
    # the rows on the grid, the planes an odd number of floats apart
    got = run_banded(hip_lib, planes, tab, per_src, md, band, ld=Na + 4, out_ld=Ta + 4, stride_extra=1)
    assert got.tobytes() == base.tobytes()
    got = run_banded(hip_lib, planes, tab, per_src, md, band, ld=Na + 4, out_ld=Ta + 4, stride_extra=3)
    assert got.tobytes() == base.tobytes()


def test_clamp_and_last_source_takes_the_rest(hip_lib):
    """Entries outside [0, max_delay] are clamped as they are loaded, and trials beyond nsrc * per_src read the last
    source."""
    planes, tab0, per_src, md, band, _ = reference("sources")
    tab = np.array(tab0)
    tab[0, 0], tab[6, 3], tab[12, 5], tab[9, 1] = -1, md + 1, (1 << 31) - 1, -(1 << 31)
    want = ref.banded(planes, tab, 4, md, band)          # per_src = 4 of 3 sources: 4, 4, 5
    got = run_banded(hip_lib, planes, tab, 4, md, band)
    assert np.array_equal(got.astype(np.float64), want)


def test_rejections_leave_the_output_untouched(hip_lib):
    import torch
    x = torch.zeros(2 * 400, dtype=torch.float32, device="cuda")
    tab = torch.zeros((3, 4), dtype=torch.int32, device="cuda")
    out = kh.GuardedOutput(6, 90, 90, 0, OUT_GUARD)
    good = ref.banded_good(x.data_ptr(), tab.data_ptr(), out.ptr)
    kh.check_rejections(hip_lib.pss_dedisperse_banded, good, ref.BANDED_REJECTIONS, prefix="dedisperse_banded")
    torch.cuda.synchronize()
    out.untouched()


# ---------------------------------------------------------------------------
# API
# ---------------------------------------------------------------------------
DMS37 = np.linspace(0.0, 60.0, 37)


def _signal(data):
    import torch
    from psrsigsim_amd.signal import FilterBankSignal
    sig = FilterBankSignal(1400, 400, Nsubband=data.shape[0], sample_rate=0.01, fold=False)
    sig._buf = torch.from_numpy(np.array(data)).cuda()
    sig._ncols = sig._nsamp = data.shape[1]
    return sig


@kh.once
def api_case(kind):
    """64 channels, N = 3 * 2048 + 5 + max delay, 37 trials: (data, direct float64 sum over the effective table)."""
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.telescope import Backend
    probe = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False)
    probe._buf, probe._ncols = object(), 1 << 20
    p = Backend.subband_plan(probe, DMS37, nsub=8, group=8)
    N = 3 * TB + 5 + p.m1 + p.m2
    if kind == "int":
        data = int_planes(1, 64, N, 30)[0]
    else:
        import torch
        data = torch.rand((64, N), dtype=torch.float32, generator=torch.Generator().manual_seed(31)).numpy()
    return data, ref.direct(data, p.delays, p.m1 + p.m2), ref.direct(np.abs(data), p.delays, p.m1 + p.m2)


def test_api_is_the_direct_sum_over_the_effective_table(hip_lib):
    import torch
    from psrsigsim_amd import _engine, _lib
    from psrsigsim_amd.telescope import DedispersedPlane, SubbandPlan
    data, want, _ = api_case("int")
    N = data.shape[1]
    sig = _signal(data)
    be = kh.backend()
    plane = be.subband_dedisperse(sig, DMS37, nsub=8, group=8)
    p = plane.subband
    assert isinstance(plane, DedispersedPlane) and isinstance(p, SubbandPlan)
    assert plane.max_delay == p.m1 + p.m2 and p.T == 3 * TB + 5 and p.d1.shape[0] == 5
    assert tuple(plane.data.shape) == (37, p.T) and plane.data.dtype == torch.float32 and plane.data.is_cuda
    assert plane.data.stride(0) % 4 == 0 and plane.data.stride(1) == 1 and plane.data.data_ptr() % 16 == 0
    assert plane.delays is p.delays and np.array_equal(plane.dms, DMS37)
    assert plane.ref_freq == 1593.75 and plane.samprate == 0.01
    got = plane.data.cpu().numpy()
    assert np.array_equal(got.astype(np.float64), want)
    # the bits of pss_dedisperse on the effective table
    tab = _engine.to_dev(plane.delays)
    x = sig.data
    out = torch.empty((37, p.T), dtype=torch.float32, device="cuda")
    _lib.check(hip_lib.pss_dedisperse(x.data_ptr(), 64, N, N, tab.data_ptr(), 37, plane.max_delay, out.data_ptr(),
                                      p.T, _engine.stream_ptr()), "dedisperse")
    assert kh.same_bits(got, out.cpu().numpy())
    assert sig.data.cpu().numpy().tobytes() == data.tobytes()           # the signal is left as it was
    # 5 groups in 3 chunks (2, 2, 1): the same bits
    per = 8 * ((p.T1 + 3) // 4 * 4) * 4
    assert be._subband_chunks(p, 2 * per + 4) == [(0, 2), (2, 4), (4, 5)]
    chunked = be.subband_dedisperse(sig, DMS37, nsub=8, group=8, max_bytes=2 * per + 4)
    assert kh.same_bits(chunked.data.cpu().numpy(), got)
    with pytest.raises(ValueError, match="one group"):
        be.subband_dedisperse(sig, DMS37, nsub=8, group=8, max_bytes=per - 1)
    # a sharded signal: this rank's partial sum over its own channels, which form the bands
    from psrsigsim_amd.signal import FilterBankSignal
    part = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False, shard=(16, 48))
    part._buf = torch.from_numpy(np.array(data[16:48])).cuda()
    part._ncols = part._nsamp = N
    pp = be.subband_dedisperse(part, DMS37, nsub=4, group=8)
    assert pp.delays.shape == (37, 32) and pp.ref_freq == 1593.75
    assert np.array_equal(pp.data.cpu().numpy().astype(np.float64), ref.direct(data[16:48], pp.delays, pp.max_delay))


def test_api_float_data_within_the_any_order_bound(hip_lib):
    """|plane - oracle64| <= C 2^-24 sum_c |x| per sample: the bound of a float32 sum of C terms in any order
    (derived, not measured)."""
    data, want, mag = api_case("float")
    plane = kh.backend().subband_dedisperse(_signal(data), DMS37, nsub=8, group=8)
    err = np.abs(plane.data.cpu().numpy().astype(np.float64) - want)
    print("float test: max err / bound", float((err / (64 * 2.0 ** -24 * mag)).max()))
    assert (err <= 64 * 2.0 ** -24 * mag).all()


def test_api_end_to_end_pulse(hip_lib):
    """make_pulses -> ISM.disperse(30) -> the two planes -> single_pulse_search: the direct plane's strongest
    candidate lies at the injected trial; the sub-band plane's at that trial +- 1 and at the same time within its
    width.  periodicity_search and fold_candidates take the plane as it stands."""
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar
    from psrsigsim_amd.ism import ISM
    pss.seed(20250101)
    sig = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False)
    Pulsar(0.05, 1.0).make_pulses(sig, tobs=1.6384)
    ISM().disperse(sig, 30)
    be = kh.backend()
    dms = np.arange(0, 65, 5)
    direct = be.dedisperse(sig, dms)
    d = be.single_pulse_search(direct, threshold=6.0).array
    top = d[np.argmax(d["snr"])]
    print("direct: strongest", top)
    assert top["dm_index"] == 6
    plane = be.subband_dedisperse(sig, dms, nsub=8, group=3)
    print(plane.subband)
    s = be.single_pulse_search(plane, threshold=6.0).array
    best = s[np.argmax(s["snr"])]
    print("sub-band: strongest", best)
    assert abs(int(best["dm_index"]) - 6) <= 1
    assert abs(int(best["time"]) - int(top["time"])) <= int(top["width"])
    cands = be.periodicity_search(plane, stat_block=128)
    assert len(cands) >= 1
    folded = be.fold_candidates(sig, candidates=cands, max_candidates=1, nbin=32, nsub=4, nband=4, stat_block=128)
    assert len(folded) == 1
