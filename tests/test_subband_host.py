"""Host side of the sub-band dedispersion (no GPU): the plan's identities
against the scalar restatement of tests/subband_ref.py, the automatic choice
against a brute-force search, every ValueError, the chunk arithmetic, the C
ABI's argument checks, and the banded kernel's index logic ported to Python
integers (every workgroup id, every global and LDS index, every output word).
"""
import numpy as np
import pytest

from psrsigsim_amd import _lib
from psrsigsim_amd.utils.constants import DM_K_VALUE
from tests import subband_ref as ref
from tests.kernel_harness import backend as _backend, check_rejections, host_pointer, once


class _StubBuf(object):
    """Stands in for the device buffer: any use of it is an error."""

    def __getattr__(self, name):
        raise AssertionError("the device buffer was touched (%s)" % name)


def _fb(nchan=64, n=16384, rate=0.01, fold=False, data=True, shard=None):
    from psrsigsim_amd._units import make_quant
    from psrsigsim_amd.signal import FilterBankSignal
    sig = FilterBankSignal(1400, 400, Nsubband=nchan, sample_rate=1000.0, fold=fold, shard=shard)
    sig._samprate = make_quant(rate, 'MHz')                    # (set here: the constructor warns below Nyquist)
    if data:
        sig._buf = _StubBuf()
        sig._ncols = sig._nsamp = n
    return sig


def _freqs(sig):
    from psrsigsim_amd._units import to_value
    return np.asarray(to_value(getattr(sig, "local_dat_freq", sig.dat_freq), 'MHz'), dtype=np.float64)


def _unrounded(sig, dms):
    f = _freqs(sig)
    fs_hz = float(sig._samprate_MHz()) * 1e6
    return DM_K_VALUE * np.asarray(dms, dtype=np.float64)[:, None] * (f ** -2.0 - f.max() ** -2.0)[None, :] * fs_hz


# (signal keywords, dms, nsub, group): the physical table, a 2048-channel one, unsorted dms
PLANS = {
    "physical": (dict(nchan=64, n=16384, rate=0.01), 5.0 * np.arange(13), 8, 4),
    "ragged": (dict(nchan=64, n=16384, rate=0.01), 5.0 * np.arange(13), 4, 5),
    "c2048": (dict(nchan=2048, n=1 << 16, rate=1.0 / 64.0), np.linspace(0.0, 100.0, 100), 64, 16),
    "unsorted": (dict(nchan=64, n=16384, rate=0.01), np.array([40.0, 0.0, 65.0, 5.0, 5.0, 33.3, 12.0, 60.0, 1.0]), 16,
                 4),
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan_identities(name):
    from psrsigsim_amd.telescope import Backend, SubbandPlan
    kw, dms, nsub, group = PLANS[name]
    sig = _fb(**kw)
    D = Backend.dedisperse_delays(sig, dms).astype(np.int64)
    p = Backend.subband_plan(sig, dms, nsub=nsub, group=group)
    assert isinstance(p, SubbandPlan) and (p.nsub, p.group) == (nsub, group)
    ndm, C = D.shape
    band, ngroups = C // nsub, -(-ndm // group)
    want = ref.plan(D, _freqs(sig), nsub, group, kw["n"])
    assert p.d1.dtype == p.d2.dtype == p.delays.dtype == np.int32
    assert p.d1.flags.c_contiguous and p.d2.flags.c_contiguous and p.delays.flags.c_contiguous
    assert p.d1.shape == (ngroups, C) and p.d2.shape == (ndm, nsub) and p.delays.shape == (ndm, C)
    for key, got in (("nominal", p.nominal), ("ref", p.ref_chan), ("d1", p.d1), ("d2", p.d2), ("e", p.delays)):
        assert np.array_equal(np.asarray(got, dtype=np.int64), want[key]), key
    assert (p.m1, p.m2, p.T1, p.T) == (want["m1"], want["m2"], want["T1"], want["T"])
    e, d1, d2 = p.delays.astype(np.int64), p.d1.astype(np.int64), p.d2.astype(np.int64)
    g_of, s_of = np.arange(ndm) // group, np.arange(C) // band
    assert np.array_equal(e, d1[g_of] + d2[:, s_of])                       # e = d1 + d2
    assert (d1 >= 0).all()
    assert p.T == kw["n"] - p.m1 - p.m2 and p.T1 == kw["n"] - p.m1
    assert p.m1 == d1.max() and p.m2 == d2.max()
    # the band's reference is its channel of largest frequency (here the last: dat_freq rises)
    assert np.array_equal(p.ref_chan, np.arange(nsub) * band + band - 1)
    smear = e - D
    assert (smear[p.nominal] == 0).all() and (smear[:, p.ref_chan] == 0).all()
    assert p.smear == np.abs(smear).max()
    x = _unrounded(sig, dms)
    delta = x[p.nominal][g_of] - x[p.nominal][g_of][:, p.ref_chan][:, s_of] + x[:, p.ref_chan][:, s_of] - x
    assert (np.abs(smear) < np.abs(delta) + 2).all()
    assert p.adds_direct == ndm * C and p.adds_subband == ngroups * C + ndm * nsub
    assert np.array_equal(p.dms, dms) and p.ref_freq == _freqs(sig).max()


def test_reference_channel_ties_and_falling_frequencies():
    """r(s) is the band's largest frequency, ties to the lowest index -- whatever the channel order."""
    from psrsigsim_amd.telescope import subband
    f = np.array([3.0, 5.0, 5.0, 1.0, 9.0, 8.0, 7.0, 6.0, 2.0, 2.0, 2.0, 2.0])
    assert subband._ref_channels(f, 3).tolist() == [1, 4, 8]
    assert subband._ref_channels(f, 1).tolist() == [4]
    assert subband._ref_channels(f, 12).tolist() == list(range(12))


def _brute_choice(sig, dms, max_smear, N):
    from psrsigsim_amd.telescope import Backend
    D = Backend.dedisperse_delays(sig, dms).astype(np.int64)
    ndm, C = D.shape
    best, reached = None, None
    nsub = 1
    while 2 * nsub <= C:
        group = 8
        while C % nsub == 0 and group <= max(8, ndm):
            p = ref.plan(D, _freqs(sig), nsub, group, N)
            smear = int(np.abs(p["e"] - D).max())
            reached = smear if reached is None else min(reached, smear)
            key = (-(-ndm // group) * C + ndm * nsub, nsub, group)
            if smear <= max_smear and (best is None or key < best):
                best = key
            group *= 2
        nsub *= 2
    return best, reached


@pytest.mark.parametrize("nchan,rate,ndm,top,max_smear", [(64, 0.01, 40, 8.0, 2.0), (64, 0.01, 40, 8.0, 1.0),
                                                          (64, 0.01, 100, 50.0, 2.0), (64, 0.01, 5, 1.0, 2.0)])
def test_automatic_choice_is_the_brute_force_optimum(nchan, rate, ndm, top, max_smear):
    from psrsigsim_amd.telescope import Backend
    N = 1 << 17
    sig = _fb(nchan=nchan, n=N, rate=rate)
    dms = np.linspace(0.0, top, ndm)
    want, _ = _brute_choice(sig, dms, max_smear, N)
    assert want is not None
    p = Backend.subband_plan(sig, dms, max_smear=max_smear)
    assert (p.adds_subband, p.nsub, p.group) == want
    assert p.smear <= max_smear and p.group % 8 == 0 and (p.nsub & (p.nsub - 1)) == 0 and 2 * p.nsub <= nchan
    # one value given: it is kept, the other chosen
    q = Backend.subband_plan(sig, dms, nsub=p.nsub, max_smear=max_smear)
    assert (q.nsub, q.group) == (p.nsub, p.group)
    q = Backend.subband_plan(sig, dms, group=8, max_smear=max_smear)
    assert q.group == 8 and q.smear <= max_smear
    # both given: used as they are, whatever the smear
    q = Backend.subband_plan(sig, dms, nsub=1, group=ndm, max_smear=0.0)
    assert (q.nsub, q.group) == (1, ndm) and q.smear > 0


def test_value_errors(monkeypatch):
    from psrsigsim_amd import _engine
    from psrsigsim_amd.signal import BasebandSignal
    from psrsigsim_amd.telescope import Backend

    def boom(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_engine, "to_dev", boom)
    monkeypatch.setattr(_engine, "execute", boom)
    be = _backend()
    dms = 5.0 * np.arange(13)
    for call in (Backend.subband_plan, be.subband_dedisperse):
        for bad in ([-1.0], [np.nan], [1.0, np.inf]):
            with pytest.raises(ValueError, match="negative or not finite"):
                call(_fb(), bad)
        with pytest.raises(ValueError, match="empty"):
            call(_fb(), [])
        with pytest.raises(ValueError, match="below a channel frequency"):
            call(_fb(), dms, ref_freq=1500.0)
        with pytest.raises(ValueError, match="int32"):
            call(_fb(), [0.0, 1e9])
        with pytest.raises(ValueError, match="fold"):
            call(_fb(fold=True), dms)
        with pytest.raises(ValueError, match="no data"):
            call(_fb(data=False), dms)
        bb = BasebandSignal(1400, 400, Nchan=2)
        bb._buf = _StubBuf()
        bb._ncols = bb._nsamp = 4096
        with pytest.raises(ValueError, match="FilterBankSignal"):
            call(bb, dms)
        for nsub in (0, -2, 3, 128, 48):
            with pytest.raises(ValueError, match="nsub %d does not divide" % nsub):
                call(_fb(), dms, nsub=nsub)
        for group in (0, -8):
            with pytest.raises(ValueError, match="group %d < 1" % group):
                call(_fb(), dms, group=group)
        with pytest.raises(ValueError, match="integers"):
            call(_fb(), dms, nsub=2.5)
        with pytest.raises(ValueError, match="integers"):
            call(_fb(), dms, group="x")
        with pytest.raises(ValueError, match="max_smear"):
            call(_fb(), dms, max_smear=-1.0)
        with pytest.raises(ValueError, match="max_smear"):
            call(_fb(), dms, max_smear=np.nan)
        # T = N - m1 - m2 >= 1: DM 60 needs 749 samples
        with pytest.raises(ValueError, match="largest delay"):
            call(_fb(n=700), dms, nsub=8, group=4)
    # no pair qualifies: 13 coarse trials of 64 channels cannot be grouped by 8 within half a sample
    _, reached = _brute_choice(_fb(), dms, 0.0, 16384)
    assert reached > 0
    with pytest.raises(ValueError, match="smallest reached is %d" % reached):
        Backend.subband_plan(_fb(), dms, max_smear=0.0)
    with pytest.raises(ValueError, match="no band of at least 2"):
        Backend.subband_plan(_fb(nchan=1), dms)
    p = Backend.subband_plan(_fb(), dms, nsub=8, group=4)
    with pytest.raises(ValueError, match="one group"):
        be.subband_dedisperse(_fb(), dms, nsub=8, group=4, max_bytes=8 * ((p.T1 + 3) // 4 * 4) * 4 - 1)
    with pytest.raises(ValueError, match="integers"):
        be.subband_dedisperse(_fb(), dms, nsub=8, group=4, max_bytes=1.5)
    # the smallest valid signal: one output sample
    p = Backend.subband_plan(_fb(n=p.m1 + p.m2 + 1), dms, nsub=8, group=4)
    assert p.T == 1


def test_chunks_of_whole_groups():
    from psrsigsim_amd.telescope import Backend
    be = _backend()
    p = Backend.subband_plan(_fb(), np.linspace(0, 60, 37), nsub=8, group=8)
    assert p.d1.shape[0] == 5
    per = 8 * ((p.T1 + 3) // 4 * 4) * 4
    assert be._subband_chunks(p, 2 ** 31) == [(0, 5)]
    assert be._subband_chunks(p, 5 * per) == [(0, 5)]
    assert be._subband_chunks(p, 5 * per - 1) == [(0, 4), (4, 5)]
    assert be._subband_chunks(p, 2 * per + 7) == [(0, 2), (2, 4), (4, 5)]          # a ragged last chunk
    assert be._subband_chunks(p, per) == [(g, g + 1) for g in range(5)]
    with pytest.raises(ValueError, match="one group"):
        be._subband_chunks(p, per - 1)


def test_entry_point_is_declared_and_validates_arguments():
    """NULL pointers and each out-of-range scalar return PSS_EINVAL with the
    argument named and no device touched."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "pss_hip.h")) as f:
        assert re.search(r"\bint pss_dedisperse_banded\(", f.read())
    p = host_pointer()
    check_rejections(_lib.load().pss_dedisperse_banded, ref.banded_good(p, p, p), ref.BANDED_REJECTIONS,
                     prefix="dedisperse_banded")


# ---------------------------------------------------------------------------
# the kernel's index logic (pss_dedisperse.hip: pss_dedisperse_banded,
# k_dedisperse_banded, dd_tile; pss_window.hpp: stage_window) in Python integers
# ---------------------------------------------------------------------------
TB, ND, CB, NJ, WIN, SPREAD, THREADS = 2048, 8, 2, 2, 4096, 2044, 256
SENT = float(1 << 20)


def port_entry(nsrc, src_stride, nchan, n, ld, ndm, per_src, max_delay, band, out_ld, base_word=0):
    """The entry point's launch arithmetic: the kernel's arguments and grid."""
    T = n - max_delay
    nsu = min(nsrc, (ndm + per_src - 1) // per_src)
    last = ndm - (nsu - 1) * per_src
    gps = (per_src + ND - 1) // ND if nsu > 1 else (last + ND - 1) // ND
    ngroups = (nsu - 1) * gps + (last + ND - 1) // ND
    nbands = (nchan + band - 1) // band
    ntiles = (T + TB - 1) // TB
    grid = ntiles * nbands * ngroups
    assert grid <= 0x7fffffff
    vec = base_word % 4 == 0 and ld % 4 == 0 and (nsu == 1 or src_stride % 4 == 0)
    return dict(n=n, ld=ld, out_ld=out_ld, T=T, nchan=nchan, ndm=ndm, max_delay=max_delay, ngroups=ngroups,
                src_stride=src_stride, band=band, nbands=nbands, per_src=per_src, nsrc=nsu, gps=gps, grid=grid, vec=vec,
                base_word=base_word)


def port_workgroup_id(bid, a):
    """blockIdx.x -> (time tile, band, source, first trial, trials): xcd_run_pair and the kernel's prologue."""
    total = a["grid"]
    base, rem, xcd = total >> 3, total & 7, bid & 7
    lid = xcd * base + min(xcd, rem) + (bid >> 3)
    slow, g = lid // a["ngroups"], lid % a["ngroups"]
    s, tile = slow % a["nbands"], slow // a["nbands"]
    q = min(g // a["gps"], a["nsrc"] - 1)
    j0 = q * a["per_src"] + (g - q * a["gps"]) * ND
    jend = a["ndm"] if q == a["nsrc"] - 1 else (q + 1) * a["per_src"]
    return tile, s, q, j0, min(ND, jend - j0)


def port_stage_window(mem, row, wb, need, a, vec):
    """stage_window<THREADS, WIN, VEC, false>: the window's words; every index asserted."""
    n = a["n"]
    assert 1 <= need <= WIN and wb >= 0 and wb + need <= n
    nq = (need + 3) >> 2
    win = np.full(WIN, np.nan)                        # (words nothing staged: stale)
    if vec and wb + 4 * nq <= n:
        assert (a["base_word"] + row + wb) % 4 == 0, "a 16-B load off the grid"
        for i in range(WIN // 4 // THREADS):
            for tid in (0, THREADS - 1):
                grp = min(tid + i * THREADS, nq - 1)
                assert 0 <= wb + 4 * grp and wb + 4 * grp + 4 <= n
                if i * THREADS < nq:
                    assert 4 * (tid + i * THREADS) + 4 <= WIN
        win[:4 * nq] = mem[row + wb:row + wb + 4 * nq]
        return win
    assert 4 * nq <= WIN
    for k in range(4 * nq):
        s = wb + k
        win[k] = mem[row + s] if s < n else 0.0
    return win


def port_kernel(mem, table, a, out, written):
    """Every workgroup of the launch; sums into ``out`` [ndm * nb][out_ld], counts the stores in ``written``."""
    n, ld, T, nchan, md = a["n"], a["ld"], a["T"], a["nchan"], a["max_delay"]
    seen = set()
    for bid in range(a["grid"]):
        tile, s, q, j0, nd = port_workgroup_id(bid, a)
        assert 0 <= s < a["nbands"] and 0 <= q < a["nsrc"] and nd >= 1 and 0 <= j0 and j0 + nd <= a["ndm"]
        t0 = tile * TB
        assert 0 <= t0 < T
        # no group straddles a source
        assert {min(j // a["per_src"], a["nsrc"] - 1) for j in range(j0, j0 + nd)} == {q}
        assert (tile, s, j0) not in seen
        seen.add((tile, s, j0))
        ln = min(TB, T - t0)
        c_lo = s * a["band"]
        c_hi = c_lo + min(a["band"], nchan - c_lo)
        assert 0 <= c_lo < c_hi <= nchan
        src = q * a["src_stride"]
        acc = np.zeros((ND, TB))
        for c0 in range(c_lo, c_hi, CB):
            for cb in range(CB):
                c = c0 + cb
                if c >= c_hi:
                    continue
                row = src + c * ld
                d = [min(max(int(table[j0 + min(j, nd - 1), c]), 0), md) for j in range(ND)]
                dmin, dmax = min(d), max(d)
                if dmax - dmin <= SPREAD:
                    ws = (t0 + dmin) & ~3
                    need = t0 + dmax - ws + ln
                    win = port_stage_window(mem, row, ws, need, a, a["vec"])
                    for j in range(ND):
                        off = t0 + d[j] - ws
                        assert off >= 0 and off + TB <= WIN
                        acc[j, :ln] += win[off:off + ln]
                else:
                    for j in range(0, ND, NJ):
                        win = np.full(WIN, np.nan)
                        for i in range(NJ):
                            lo = t0 + d[j + i]
                            assert 0 <= lo and lo + ln <= n and i * TB + ln <= WIN
                            win[i * TB:i * TB + ln] = mem[row + lo:row + lo + ln]
                        for i in range(NJ):
                            assert i * TB + TB <= WIN
                            acc[j + i, :ln] += win[i * TB:i * TB + ln]
        o0, orow = (j0 * a["nbands"] + s) * a["out_ld"], a["nbands"] * a["out_ld"]
        for j in range(nd):
            lo = o0 + j * orow + t0
            assert lo + ln <= out.size
            out[lo:lo + ln] = acc[j, :ln]
            written[lo:lo + ln] += 1
    return len(seen)


def _random_launch(rng, k):
    nsrc = int(rng.integers(1, 5))
    nchan = int(rng.integers(1, 12))
    band = int(rng.integers(1, nchan + 2))
    ndm = int(rng.integers(1, 30))
    per_src = int(rng.choice([1, 3, 5, 8, 9, 16, 17, ndm, ndm + 3]))
    wide = k % 3 == 0
    md = int(rng.integers(2100, 3000)) if wide else int(rng.integers(0, 60))
    n = md + int(rng.choice([1, 7, TB - 1, TB, TB + 1, 2 * TB + 5]))
    ld = n + int(rng.integers(0, 6))
    src_stride = nchan * ld + int(rng.integers(0, 9))
    T = n - md
    out_ld = T + int(rng.integers(0, 4))
    table = rng.integers(-3, md + 4, size=(ndm, nchan))
    base_word = int(rng.integers(0, 4)) if k % 2 else 0
    return nsrc, src_stride, nchan, n, ld, ndm, per_src, md, band, out_ld, table, base_word


@pytest.mark.parametrize("seed", range(4))
def test_kernel_port_stays_in_bounds_and_gives_the_definition(seed):
    rng = np.random.default_rng(100 + seed)
    for k in range(9):
        nsrc, src_stride, nchan, n, ld, ndm, per_src, md, band, out_ld, table, base_word = _random_launch(rng, k)
        a = port_entry(nsrc, src_stride, nchan, n, ld, ndm, per_src, md, band, out_ld, base_word)
        planes = rng.integers(0, 16, size=(nsrc, nchan, n)).astype(np.float64)
        mem = np.full(nsrc * src_stride, SENT)            # every word outside a row's [0, n): the sentinel
        for q in range(nsrc):
            for c in range(nchan):
                mem[q * src_stride + c * ld:q * src_stride + c * ld + n] = planes[q, c]
        nb = a["nbands"]
        out = np.full(ndm * nb * out_ld, -7.0)
        written = np.zeros(out.size, dtype=np.int64)
        nwg = port_kernel(mem, table, a, out, written)
        assert nwg == a["grid"]                           # every id is one (tile, band, source, group)
        w = written.reshape(ndm * nb, out_ld)
        assert (w[:, :a["T"]] == 1).all() and (w[:, a["T"]:] == 0).all()      # every output word exactly once
        want = ref.banded(planes, table, per_src, md, band)
        assert np.array_equal(out.reshape(ndm, nb, out_ld)[:, :, :a["T"]], want), (seed, k)


def test_port_with_one_source_and_one_band_is_the_direct_sum():
    rng = np.random.default_rng(5)
    planes = rng.integers(0, 16, size=(1, 5, 2300)).astype(np.float64)
    table = rng.integers(0, 41, size=(11, 5))
    a = port_entry(1, 5 * 2304, 5, 2300, 2304, 11, 11, 40, 5, 2260)
    assert (a["nbands"], a["nsrc"], a["ngroups"], a["grid"], a["vec"]) == (1, 1, 2, 4, True)
    mem = np.full(5 * 2304, SENT)
    for c in range(5):
        mem[c * 2304:c * 2304 + 2300] = planes[0, c]
    out, written = np.full(11 * 2260, -7.0), np.zeros(11 * 2260, dtype=np.int64)
    port_kernel(mem, table, a, out, written)
    assert (written == 1).all()
    assert np.array_equal(out.reshape(11, 2260), ref.direct(planes[0], table, 40))


@once
def _stage_tables():
    from psrsigsim_amd.telescope import Backend
    sig = _fb(n=3 * 2048 + 5 + 800)
    return Backend.subband_plan(sig, np.linspace(0, 60, 37), nsub=8, group=8)


def test_the_two_stages_as_banded_launches_give_the_plane():
    """The API's two launches per chunk, through the port's entry arithmetic: stage 2 of 5 sources owns trial groups of
    8, 8, 8, 8, 5, and the composition is the direct sum over the effective table."""
    p = _stage_tables()
    a = port_entry(5, 8 * p.T1, 8, p.T1, p.T1, 37, 8, p.m2, 8, p.T)
    assert (a["nsrc"], a["gps"], a["ngroups"], a["nbands"]) == (5, 1, 5, 1)
    ids = [port_workgroup_id(b, a) for b in range(a["grid"])]
    assert sorted(i[2:] for i in ids if i[0] == 0) == [(0, 0, 8), (1, 8, 8), (2, 16, 8), (3, 24, 8), (4, 32, 5)]
    rng = np.random.default_rng(8)
    N = p.T + p.m1 + p.m2
    data = rng.integers(0, 16, size=(64, N)).astype(np.float64)
    tabs = dict(d1=p.d1.astype(np.int64), d2=p.d2.astype(np.int64), T1=p.T1, T=p.T)
    assert np.array_equal(ref.two_stage(data, tabs, 8, 8), ref.direct(data, p.delays, p.m1 + p.m2))
    s1 = ref.banded(data[None], p.d1, 5, p.m1, 8)
    assert np.array_equal(ref.banded(s1, p.d2, 8, p.m2, 8)[:, 0], ref.direct(data, p.delays, p.m1 + p.m2))
