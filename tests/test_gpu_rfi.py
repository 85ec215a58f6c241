"""RFI excision on the GPU (``pss_rfi_clean``, ``Backend.rfi_stats`` / ``rfi_mask`` / ``rfi_clean``).

The models are tests/rfi_ref.py: ``clean`` restates the kernel in float32 operation for operation in its
documented summation order (8 contiguous channel ranges, each in increasing c, combined in a fixed tree), and
``mask_rule`` the mask's four rules in float64.

Kernel cases use integer-valued data and ``base`` (seeded integers 0..15): every partial sum of
``data - base`` is then an exact float32 in any order, and the comparison with the float32 model is bitwise.
Every flagged cell of the input holds 1e30 (it must reach no output), the input lies inside a larger tensor
whose every other word holds 2^20 (a stray read lands in a sum) and the outputs inside tensors of a guard
value that is checked afterwards (tests/kernel_harness.py).

The kernel's tile (pss_rficlean.hip): a workgroup owns TILE = 256 times of every channel; a tile that lies
inside one block of the mask takes the wave-uniform path, one that straddles a border the per-lane lookup.
"""
import numpy as np
import pytest

from tests import kernel_harness as kh
from tests import rfi_ref
from tests.kernel_harness import engine_seed_restored  # noqa: F401 (autouse here)

pytestmark = pytest.mark.gpu

TILE = 256
IN_GUARD = float(1 << 20)
POISON = np.float32(1e30)

# name: (C, N, block, fully flagged block or None)
CASES = {
    "degenerate": (1, 64, 16, None),               # one channel: a flagged cell leaves its block without a good one
    "odd": (3, 1000, 37, None),                    # borders off the 4-sample grid, a ragged tail of 1 in the last block
    "allflag": (5, 700, 64, 4),                    # block 4 entirely flagged: rgood = 0, the block comes out as base
    "c67": (67, 4096, 64, None),                   # a channel count that is no multiple of the split (ranges of 9, 9, .., 4)
    "channels": (4096, 2048, 256, None),           # many channels; every tile inside one block (the uniform path)
    "ragged": (9, TILE + 1, 32, None),             # one time tile + 1 sample
    "runs12": (6, 11 * TILE + 5, 100, None),       # 12 workgroups: more than the 8 XCDs and no multiple of 8
    "uniform": (13, 3000, 512, 2),                 # tiles inside one block, the last two in the clamped ragged tail
}


@kh.once
def case(name):
    """(x [C][N] with 1e30 in the flagged cells, mask uint8 [nblk][C], block, base, rgood, {zero_dm: (out, z)})."""
    C, N, block, full = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 100)
    nblk = N // block
    mask = (rng.random((nblk, C)) < 0.3).astype(np.uint8)
    if full is not None:
        mask[full, :] = 1
    x = rng.integers(0, 16, size=(C, N)).astype(np.float32)
    x[mask[rfi_ref.sample_blocks(N, block, nblk), :].T != 0] = POISON
    base = rng.integers(0, 16, size=C).astype(np.float32)
    good = C - mask.sum(axis=1)
    rgood = np.where(good > 0, 1.0 / np.maximum(good, 1), 0.0).astype(np.float32)
    ref = {zd: rfi_ref.clean(x, mask, block, base, rgood, zd) for zd in (0, 1)}
    return x, mask, block, base, rgood, ref


def run_kernel(hip_lib, x, mask, block, base, rgood, zero_dm, ld=None, out_ld=None, in_off=0, out_off=0,
               inplace=False, series=True):
    """pss_rfi_clean on guarded views.  Returns (out [C][N], z [N] or None) after checking that nothing but
    out[c][0 .. N) and zser[0 .. N) was written (zser: not at all when it is not asked for or zero_dm = 0)."""
    import torch
    from psrsigsim_amd import _lib
    C, N = x.shape
    ld = (N + 3) // 4 * 4 + 4 if ld is None else ld
    out_ld = (N + 3) // 4 * 4 + 8 if out_ld is None else out_ld
    xin = kh.GuardedInput(x, ld, in_off, IN_GUARD)
    out = kh.GuardedOutput(C, N, out_ld, out_off)
    zs = kh.GuardedOutput(1, N)
    dm = torch.from_numpy(np.array(mask, dtype=np.uint8)).cuda()
    db, dr = torch.from_numpy(np.array(base)).cuda(), torch.from_numpy(np.array(rgood)).cuda()
    before = xin.parent.clone()
    rc = hip_lib.pss_rfi_clean(xin.ptr, C, N, ld, dm.data_ptr(), block, mask.shape[0], db.data_ptr(),
                               dr.data_ptr() if zero_dm else None, zero_dm, xin.ptr if inplace else out.ptr,
                               ld if inplace else out_ld, zs.ptr if series else None, None)
    _lib.check(rc, "rfi_clean")
    torch.cuda.synchronize()
    if inplace:
        got = xin.view[:, :N].cpu().numpy().copy()
        out.untouched()
        xin.view[:, :N] = torch.from_numpy(np.array(x)).cuda()
    else:
        got = out.read()
    assert torch.equal(xin.parent.view(torch.int32), before.view(torch.int32)), \
        "the input (in place: anything but its rows' valid part) was written"
    if series and zero_dm:
        return got, zs.read()[0]
    zs.untouched()
    return got, None


@pytest.mark.parametrize("zero_dm", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_equal_the_model(name, zero_dm, hip_lib):
    """Bitwise equal to the float32 model; the same bits with zser NULL, in place and on a second run."""
    x, mask, block, base, rgood, ref = case(name)
    want, wz = ref[zero_dm]
    assert not (want == POISON).any() and np.isfinite(want).all()
    got, z = run_kernel(hip_lib, x, mask, block, base, rgood, zero_dm)
    assert kh.same_bits(got, want)
    if zero_dm:
        assert kh.same_bits(z, wz)
        full = CASES[name][3]
        if full is not None:                                   # rgood = 0: z = 0 and the block is base
            blk = slice(full * block, (full + 1) * block)
            assert not z[blk].any() and np.array_equal(got[:, blk], np.repeat(base[:, None], block, axis=1))
    noz, none = run_kernel(hip_lib, x, mask, block, base, rgood, zero_dm, series=False)
    assert none is None and kh.same_bits(noz, got)
    inp, zi = run_kernel(hip_lib, x, mask, block, base, rgood, zero_dm, inplace=True)
    assert kh.same_bits(inp, got) and (zi is None or kh.same_bits(zi, z))
    again, za = run_kernel(hip_lib, x, mask, block, base, rgood, zero_dm)
    assert kh.same_bits(again, got) and (za is None or kh.same_bits(za, z))


@pytest.mark.parametrize("zero_dm", [0, 1])
@pytest.mark.parametrize("name", ["odd", "c67", "ragged", "uniform"])
def test_misaligned_views_give_the_same_bits(name, zero_dm, hip_lib):
    """data base off by one float and an odd ld (dword loads), out off by one float and an odd out_ld (dword
    stores), each alone and together, out of place and in place: the bits of the aligned run."""
    x, mask, block, base, rgood, ref = case(name)
    N = x.shape[1]
    Na = (N + 3) // 4 * 4
    aligned, z = run_kernel(hip_lib, x, mask, block, base, rgood, zero_dm, ld=Na + 4, out_ld=Na + 4)
    assert kh.same_bits(aligned, ref[zero_dm][0])
    for kw in kh.misaligned_layouts(Na + 4, Na + 4, kh.odd(N + 2), kh.odd(N + 2)):
        got, gz = run_kernel(hip_lib, x, mask, block, base, rgood, zero_dm, **kw)
        assert kh.same_bits(got, aligned), kw
        assert gz is None or kh.same_bits(gz, z), kw
    inp, _ = run_kernel(hip_lib, x, mask, block, base, rgood, zero_dm, ld=kh.odd(N + 2), in_off=1, inplace=True)
    assert kh.same_bits(inp, aligned)


@pytest.mark.parametrize("name", ["odd", "uniform"])
def test_nan_in_a_good_cell_stays_at_its_sample(name, hip_lib):
    """A NaN in a good cell reaches z[t] and sample t of every good channel, nothing else; without zero_dm its
    own cell only.  (The flagged cells hold 1e30 throughout.)"""
    x, mask, block, base, rgood, ref = case(name)
    C, N = x.shape
    good = mask[rfi_ref.sample_blocks(N, block, mask.shape[0]), :].T == 0
    c, t = [int(v[0]) for v in np.nonzero(good & (np.arange(N) > N // 2)[None, :])]
    xn = np.array(x)
    xn[c, t] = np.nan
    for zero_dm in (0, 1):
        got, z = run_kernel(hip_lib, xn, mask, block, base, rgood, zero_dm)
        want = np.zeros((C, N), dtype=bool)
        if zero_dm:
            want[:, t] = good[:, t]
            assert np.array_equal(np.flatnonzero(np.isnan(z)), [t])
        else:
            want[c, t] = True
        assert np.array_equal(np.isnan(got), want)
        assert np.array_equal(got[~want], ref[zero_dm][0][~want])


def test_float_data_within_the_sequential_sum_bound(hip_lib):
    """chisquare(4) / 4 data and a float base, 67 channels: against the float64 model of the same order,

        |z - z64|     <= (C + 2) u B,   B = rgood * sum_{c good} |x - base|,  u = 2^-24
        |out - out64| <= (C + 2) u B + u |out64| (1 + 2^-20)

    Derived, not tuned: a term passes one subtraction, at most ceil(C / 8) - 1 additions of its range, 3 of
    the tree and the multiplication -- ceil(C / 8) + 4 <= C + 2 roundings for C >= 3, each (1 + d), |d| <= u,
    to first order; (C + 2) u covers the higher orders ((1 + u)^13 - 1 < 69 u).  The output adds the
    rounding of one subtraction, u |x - z| <= u (|out64| + |z - z64|)."""
    C, N, block = 67, 4096, 64
    _, mask, _, _, rgood, _ = case("c67")
    rng = np.random.default_rng(67)
    x = (rng.chisquare(4, size=(C, N)) / 4).astype(np.float32)
    base = rng.uniform(0.9, 1.1, size=C).astype(np.float32)
    o64, z64 = rfi_ref.clean64(x, mask, block, base, rgood, 1)
    bt = rfi_ref.sample_blocks(N, block, mask.shape[0])
    good = mask[bt, :].T == 0
    B = (np.abs(x.astype(np.float64) - base.astype(np.float64)[:, None]) * good).sum(axis=0) * rgood.astype(np.float64)[bt]
    u = 2.0 ** -24
    got, z = run_kernel(hip_lib, x, mask, block, base, rgood, 1)
    ez = np.abs(z.astype(np.float64) - z64)
    eo = np.abs(got.astype(np.float64) - o64)
    bo = (C + 2) * u * B[None, :] + u * np.abs(o64) * (1 + 2.0 ** -20)
    print("z: max err / bound", float((ez / ((C + 2) * u * B)).max()), "out: max err / bound",
          float((eo[good] / bo[good]).max()))
    assert (ez <= (C + 2) * u * B).all()
    assert (eo[good] <= bo[good]).all() and np.array_equal(got[~good], np.broadcast_to(base[:, None], (C, N))[~good])
    # the float32 model restates the kernel operation for operation
    o32, z32 = rfi_ref.clean(x, mask, block, base, rgood, 1)
    assert kh.same_bits(got, o32) and kh.same_bits(z, z32)


# ---------------------------------------------------------------------------
# API
# ---------------------------------------------------------------------------
def _signal(x, rate=0.01):
    import torch
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd._units import make_quant
    sig = FilterBankSignal(1400, 400, Nsubband=x.shape[0], sample_rate=rate, fold=False)
    sig._buf = torch.from_numpy(np.array(x)).cuda()
    sig._ncols = sig._nsamp = x.shape[1]
    sig._tobs = make_quant(x.shape[1] / (rate * 1e6), 's')
    sig._sublen, sig._nsub = sig._tobs, 1
    return sig


@kh.once
def mask_reference():
    x, inj = rfi_ref.mask_case(0)
    return x, inj, rfi_ref.mask_rule(x, block=rfi_ref.MASK_CASE_BLOCK)


def test_mask_case_equals_the_rule(hip_lib):
    """The issue's mask case (64 x 32868, blocks of 256: tone, gain burst, broadband impulse, narrow burst): the
    device mask equals the float64 model cell for cell, holds every injected cell and at most 8 of the 8192
    cells beyond them; base and rgood equal the model's.  First, on the model: no comparison lies within 1e-6
    (relative) of its threshold, so the last bits of the device's float64 sums and sqrt cannot flip a flag."""
    import torch
    from psrsigsim_amd.telescope import RfiMask
    x, inj, r = mask_reference()
    assert r["margin"] > 1e-6
    sig = _signal(x)
    be = kh.backend()
    block = rfi_ref.MASK_CASE_BLOCK
    m, v = be.rfi_stats(sig, block=block)
    assert m.dtype == v.dtype == torch.float64 and tuple(m.shape) == tuple(v.shape) == (128, 64) and m.is_cuda
    ms, ss, _ = rfi_ref.block_stats(x, block)
    np.testing.assert_allclose(m.cpu().numpy(), ms, rtol=1e-13, atol=0)
    np.testing.assert_allclose(np.sqrt(np.maximum(v.cpu().numpy(), 0)), ss, rtol=1e-10, atol=0)
    mk = be.rfi_mask(sig, block=block)
    assert isinstance(mk, RfiMask) and mk.block == block and mk.nsamp == x.shape[1]
    assert mk.mask.dtype == torch.bool and mk.mask.is_cuda and tuple(mk.mask.shape) == (128, 64)
    got = mk.mask.cpu().numpy()
    assert np.array_equal(got, r["mask"])
    assert (got | ~inj).all()
    extra = int((got & ~inj).sum())
    print(mk, "extra cells", extra)
    assert extra <= 8
    assert mk.base.dtype == torch.float32 and mk.rgood.dtype == torch.float32
    assert np.array_equal(mk.rgood.cpu().numpy(), r["rgood"])
    # (the base is a median of float64 means whose last bits may differ from the model's sums: one float32 ulp)
    np.testing.assert_allclose(mk.base.cpu().numpy(), r["base"], rtol=2.0 ** -23, atol=0)
    assert mk.zapped_chans().tolist() == [5] and abs(mk.frac - got.mean()) < 1e-15
    assert np.array_equal(mk.chan_frac.cpu().numpy(), got.mean(axis=0))
    assert np.array_equal(mk.block_frac.cpu().numpy(), got.mean(axis=1))
    # zaps are OR-ed in
    zk = be.rfi_mask(sig, block=block, zap_chans=[0, 63], zap_blocks=[127]).mask.cpu().numpy()
    want = rfi_ref.mask_rule(x, block=block, zap_chans=[0, 63], zap_blocks=[127])["mask"]
    assert np.array_equal(zk, want) and zk[:, 0].all() and zk[:, 63].all() and zk[127].all()


def test_api_clean(hip_lib):
    """rfi_clean on the mask case with the device's own mask: the float32 model's bits (zero_dm 0 and 1), a
    new signal on the 16-B grid with the metadata of the old one, in place, the series, a shard."""
    import torch
    from psrsigsim_amd.signal import FilterBankSignal
    x, inj, r = mask_reference()
    N = x.shape[1]
    block = rfi_ref.MASK_CASE_BLOCK
    be = kh.backend()
    sig = _signal(x)
    mk = be.rfi_mask(sig, block=block)
    mask, base, rgood = mk.mask.cpu().numpy(), mk.base.cpu().numpy(), mk.rgood.cpu().numpy()
    for zero_dm in (True, False):
        want, wz = rfi_ref.clean(x, mask, block, base, rgood, int(zero_dm))
        new, z = be.rfi_clean(sig, mk, zero_dm=zero_dm, return_series=True)
        assert isinstance(new, FilterBankSignal) and new is not sig and not new.fold
        d = new.data
        assert tuple(d.shape) == x.shape and d.dtype == torch.float32 and d.is_cuda
        assert d.stride(0) % 4 == 0 and d.stride(1) == 1 and d.data_ptr() % 16 == 0
        assert kh.same_bits(d.cpu().numpy(), want) and kh.same_bits(z.cpu().numpy(), wz)
        assert sig.data.cpu().numpy().tobytes() == x.tobytes()                  # the signal is left as it was
        for attr in ("fcent", "bw", "samprate", "tobs", "sublen", "nsub", "Nchan", "nsamp", "shard"):
            assert getattr(new, attr) == getattr(sig, attr), attr
        assert np.array_equal(new.dat_freq.value, sig.dat_freq.value)
        assert be.rfi_clean(sig, mk, zero_dm=zero_dm).data.cpu().numpy().tobytes() == want.tobytes()
    # the tone's channel and the impulse's block are the baseline; the impulse is gone from the series
    want, wz = rfi_ref.clean(x, mask, block, base, rgood, 1)
    assert (want[5] == base[5]).all() and (want[:, 70 * block:71 * block] == base[:, None]).all()
    assert not wz[70 * block:71 * block].any() and np.abs(wz).max() < 0.5
    # in place: the signal itself
    twin = _signal(x)
    same = be.rfi_clean(twin, mk, inplace=True)
    assert same is twin and twin.data.cpu().numpy().tobytes() == want.tobytes()
    # a shard: mask replacement only
    part = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False, shard=(16, 48))
    part._buf = torch.from_numpy(np.array(x[16:48])).cuda()
    part._ncols = part._nsamp = N
    pm = be.rfi_mask(part, block=block)
    assert tuple(pm.mask.shape) == (128, 32)
    with pytest.raises(ValueError, match="whole band"):
        be.rfi_clean(part, pm)
    pc = be.rfi_clean(part, pm, zero_dm=False)
    pw, _ = rfi_ref.clean(x[16:48], pm.mask.cpu().numpy(), block, pm.base.cpu().numpy(), pm.rgood.cpu().numpy(), 0)
    assert pc.shard == (16, 48) and pc.data.cpu().numpy().tobytes() == pw.tobytes()


IMPULSES = [(t0, 16, 2.5) for t0 in (9000, 30011, 52345, 77777, 101010, 120000)]
TONE = (5, 0.5)
DMS13 = np.arange(0, 65, 5)


def test_end_to_end_search_finds_the_pulsar_after_cleaning(hip_lib, tmp_path):
    """make_pulses (P = 50 ms) -> ISM.disperse(30) -> + chisquare(4) / 4 noise -> inject_rfi (six zero-DM impulses
    of +2.5 over 16 samples, a tone of +0.5 on channel 5); 64 channels, 1200-1600 MHz, 10 kHz, N = 2^17;
    trials DM 0, 5, .. 60; single_pulse_search at threshold 8.

    CPU study (tests/rfi_ref.py and tests/pulse_search_ref.py on a NumPy analogue of the signal -- Gaussian
    profile x chisquare(1), integer delays -- seeds 0 .. 5): raw, the strongest cell is an impulse at trial 0
    with S/N 84.1 - 85.2 (the pulsar's trial reaches 21.8 - 23.2); the mask flags 1.6 % of the cells, channel
    5 whole; cleaned, the strongest cell is at trial 6 (DM 30) with S/N 19.7 - 20.1, trials 5 and 7 reach 18.8
    - 19.5 and every other trial at most 17.6, and trial 0 holds nothing above 6.15 anywhere (3.4 - 6.15 at the
    impulses).  The device draws from another generator, so asserted is only the outcome: raw, the strongest
    candidate sits at trial 0 on an impulse; cleaned, it sits within one trial of DM 30 and no candidate of
    trial 0 touches an impulse; and the cleaned signal passes dedisperse, fold_candidates and search-mode
    PSRFITS.save."""
    import torch
    import psrsigsim_amd as pss
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.pulsar import Pulsar
    from psrsigsim_amd.ism import ISM
    from psrsigsim_amd.io import PSRFITS, read_search_data
    from psrsigsim_amd.telescope import inject_rfi
    pss.seed(20250101)
    N = 1 << 17
    sig = FilterBankSignal(1400, 400, Nsubband=64, sample_rate=0.01, fold=False)
    psr = Pulsar(0.05, 1.0)
    psr.make_pulses(sig, tobs=N / 1e4)
    ISM().disperse(sig, 30)
    assert tuple(sig.data.shape) == (64, N)
    g = torch.Generator(device="cuda").manual_seed(20250101)
    for _ in range(4):
        sig.data.add_(torch.randn((64, N), dtype=torch.float32, device="cuda", generator=g).square_().mul_(0.25))
    inject_rfi(sig, tones=[TONE], impulses=IMPULSES)
    be = kh.backend()

    def touches_an_impulse(c):
        return any(c["time"] < t0 + w and t0 < c["time"] + c["width"] for t0, w, _ in IMPULSES)

    raw = be.single_pulse_search(be.dedisperse(sig, DMS13), threshold=8.0)
    top = raw.array[np.argmax(raw.snr)]
    print("raw: %d candidates, strongest" % len(raw), top)
    assert top["dm_index"] == 0 and touches_an_impulse(top)

    mk = be.rfi_mask(sig)
    clean = be.rfi_clean(sig, mk)
    print(mk)
    assert 5 in mk.zapped_chans().tolist() and mk.frac < 0.1
    plane = be.dedisperse(clean, DMS13)
    got = be.single_pulse_search(plane, threshold=8.0)
    top = got.array[np.argmax(got.snr)]
    at0 = got.array[got.dm_index == 0]
    print("clean: %d candidates, strongest" % len(got), top, "at trial 0:", len(at0))
    assert abs(int(top["dm_index"]) - 6) <= 1
    assert not any(touches_an_impulse(c) for c in at0)
    # the cleaned signal is an ordinary search-mode signal
    fc = be.fold_candidates(clean, dms=[0, 30, 60], periods=[0.05] * 3, nbin=32, nsub=4, nband=4)
    res = fc.refine()
    print("fold chi2", res["chi2"])
    assert np.isfinite(res["chi2"]).all() and int(np.argmax(res["chi2"])) == 1
    path = str(tmp_path / "clean.fits")
    PSRFITS(path, obs_mode="SEARCH").save(clean, psr, nbits=2, nsblk=4096)
    codes, values, prim, sub = read_search_data(path)
    assert codes.shape == (64, N) and prim["OBS_MODE"] == "SEARCH" and sub["NBITS"] == 2 and sub["DM"] == 30.0
