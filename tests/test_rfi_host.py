"""Host side of the RFI stage (no GPU): the mask rules on the constructed input (the float64 model of
tests/rfi_ref.py, and the stage's torch rules run on the CPU against it), the float32 model of the cleaner on a
case worked by hand, every Python-level rejection (nothing reaches the device), the C ABI's argument checks,
which precede any launch, and ``inject_rfi``'s index checks."""
import ctypes
import os

import numpy as np
import pytest

from psrsigsim_amd import _lib
from tests import rfi_ref
from tests.kernel_harness import backend as _backend, check_rejections, host_pointer


class _StubBuf(object):
    """Stands in for the device buffer: any use of it is an error."""

    def __getattr__(self, name):
        raise AssertionError("the device buffer was touched (%s)" % name)


def _fb(nchan=64, n=16384, rate=0.01, fold=False, data=True, shard=None):
    from psrsigsim_amd.signal import FilterBankSignal
    sig = FilterBankSignal(1400, 400, Nsubband=nchan, sample_rate=rate, fold=fold, shard=shard)
    if data:
        sig._buf = _StubBuf()
        sig._ncols = n
        sig._nsamp = n
    return sig


def _mask(nb=16, C=64, block=1024, nsamp=16384):
    import torch
    from psrsigsim_amd.telescope import RfiMask
    return RfiMask(torch.zeros((nb, C), dtype=torch.bool), block, nsamp, torch.zeros(C), torch.full((nb,), 1.0 / C))


def test_mask_rule_on_the_constructed_input():
    """The issue's mask case at seed 0: every injected cell is flagged, at most 8 of the 8192 cells beyond them,
    no comparison within 1e-6 (relative) of its threshold; the injected cells stand at >= 24 sigma, the tone at
    ~100 sigma_e, every clean cell below 5.9 sigma.  The stage's own rules (torch, here on the CPU, from the
    same float64 statistics) give the model's mask, base and rgood exactly."""
    import torch
    from psrsigsim_amd.telescope import rfi
    x, inj = rfi_ref.mask_case(0)
    block = rfi_ref.MASK_CASE_BLOCK
    r = rfi_ref.mask_rule(x, block=block)
    mask = r["mask"]
    assert mask.shape == inj.shape == (128, 64)
    assert (mask | ~inj).all()
    extra = int((mask & ~inj).sum())
    worst = r["cell_sigma"].max(axis=0)
    others = np.arange(64) != 5
    print("extra", extra, "margin", r["margin"], "tone", r["chan_sigma"][0, 5],
          "weakest injected cell", np.where(inj, worst, np.inf)[:, others].min(), "largest clean cell",
          np.where(inj, 0, worst).max())
    assert extra <= 8
    assert r["margin"] > 1e-6
    assert r["chan_sigma"][0, 5] > 50 and np.where(inj, worst, np.inf)[:, others].min() >= 24
    assert np.where(inj, 0, worst).max() < 5.9
    assert np.array_equal(np.flatnonzero(mask.all(axis=0)), [5]) and np.array_equal(np.flatnonzero(mask.all(axis=1)), [70])
    m, s, nb = rfi_ref.block_stats(x, block)
    xb = x.astype(np.float64)[:, :nb * block].reshape(64, nb, block)
    mt = torch.from_numpy(xb.sum(axis=2).T / block)
    vt = torch.from_numpy((xb * xb).sum(axis=2).T / block) - mt * mt
    got = rfi._mask_rules(mt, vt, 5.0, 5.0, 17 // 2, 0.5, 0.5, [], [])
    assert np.array_equal(got.numpy(), mask)
    base, rgood = rfi._mask_tables(got, mt)
    assert base.dtype == torch.float32 and np.array_equal(base.numpy(), r["base"])
    assert rgood.dtype == torch.float32 and np.array_equal(rgood.numpy(), r["rgood"])
    assert r["rgood"][70] == 0 and r["rgood"][0] == np.float32(1.0 / 63)


def test_mask_rule_zaps_fractions_and_degenerate_statistics():
    """sigma = 0 flags exactly the cells that differ; a non-finite statistic is flagged; zaps are OR-ed in; the
    fractions of rule 4 come from the flags of rules 1-3 (not cascaded)."""
    import torch
    from psrsigsim_amd.telescope import rfi
    x = np.ones((8, 16 * 16), dtype=np.float32)
    x[2, 3 * 16 + 5] = 2.0                                   # one cell that differs, sigma = 0
    x[4, 7 * 16] = np.nan                                    # one non-finite statistic
    kw = dict(block=16, chan_window=3, chanfrac=0.5, intfrac=0.2)
    r = rfi_ref.mask_rule(x, zap_chans=[6], zap_blocks=[9], **kw)
    f = np.zeros((16, 8), dtype=bool)
    f[3, 2] = f[7, 4] = True
    f[:, 6] = True
    f[9, :] = True
    assert np.array_equal(r["flags"], f)
    want = f.copy()
    want[3, :] = want[7, :] = True                           # 2 of 8 channels > 0.2: the block goes
    assert np.array_equal(r["mask"], want)                   # (channels 2 and 4 stay below chanfrac)
    assert r["base"][4] == 1.0 and r["rgood"][3] == 0 and r["rgood"][0] == np.float32(1.0 / 7)
    m, s, nb = rfi_ref.block_stats(x, 16)
    mt = torch.from_numpy(m)
    vt = torch.from_numpy(np.where(np.isfinite(s), s * s, np.nan))
    got = rfi._mask_rules(mt, vt, 5.0, 5.0, 1, 0.5, 0.2, [6], [9])
    assert np.array_equal(got.numpy(), want)


def test_clean_model_by_hand():
    """3 channels x 6 samples, blocks of 2 (3 blocks; nblk = 2 puts samples 4, 5 into block 1)."""
    x = np.array([[1, 2, 3, 4, 5, 6], [10, 10, 10, 10, 10, 10], [0, 1, 0, 1, 0, 1]], dtype=np.float32)
    mask = np.array([[0, 1, 0], [0, 0, 1]], dtype=np.uint8)
    base = np.array([1, 10, 0.5], dtype=np.float32)
    rgood = np.array([0.5, 0.5], dtype=np.float32)
    out, z = rfi_ref.clean(x, mask, 2, base, rgood, 0)
    assert np.array_equal(out, [[1, 2, 3, 4, 5, 6], [10, 10, 10, 10, 10, 10], [0, 1, 0.5, 0.5, 0.5, 0.5]])
    assert not z.any()
    out, z = rfi_ref.clean(x, mask, 2, base, rgood, 1)
    # S: block 0 sums channels 0 and 2, block 1 channels 0 and 1
    assert np.array_equal(z, [-0.25, 0.75, 1, 1.5, 2, 2.5])
    assert np.array_equal(out[0], x[0] - z) and np.array_equal(out[1], [10, 10, 9, 8.5, 8, 7.5])
    assert np.array_equal(out[2], [0.25, 0.25, 0.5, 0.5, 0.5, 0.5])
    # a flagged NaN reaches nothing; a good NaN its own sample of the good channels only
    x2 = x.copy()
    x2[1, 0] = np.nan
    x2[2, 5] = 1e30
    assert np.array_equal(rfi_ref.clean(x2, mask, 2, base, rgood, 1)[0], out)
    x2[0, 3] = np.nan
    o3, z3 = rfi_ref.clean(x2, mask, 2, base, rgood, 1)
    bad = np.isnan(o3)
    assert np.array_equal(np.argwhere(bad), [[0, 3], [1, 3]]) and np.array_equal(np.flatnonzero(np.isnan(z3)), [3])
    assert np.array_equal(o3[~bad], out[~bad])
    o64, z64 = rfi_ref.clean64(x, mask, 2, base, rgood, 1)
    assert o64.dtype == np.float64 and np.array_equal(o64, out) and np.array_equal(z64, z)


def test_rejections_never_reach_the_device(monkeypatch):
    import torch
    from psrsigsim_amd import _engine
    from psrsigsim_amd.signal import BasebandSignal
    from psrsigsim_amd.telescope import RfiMask

    def boom(*a, **k):
        raise AssertionError("the device was reached")

    monkeypatch.setattr(_lib, "lib", boom)
    monkeypatch.setattr(_engine, "to_dev", boom)
    monkeypatch.setattr(_engine, "execute", boom)
    be = _backend()
    bb = BasebandSignal(1400, 400, Nchan=2)
    bb._buf = _StubBuf()
    bb._ncols = bb._nsamp = 4096
    for call in (lambda s: be.rfi_stats(s), lambda s: be.rfi_mask(s), lambda s: be.rfi_clean(s, _mask())):
        with pytest.raises(ValueError, match="fold"):
            call(_fb(fold=True))
        with pytest.raises(ValueError, match="FilterBankSignal"):
            call(bb)
        with pytest.raises(ValueError, match="no data"):
            call(_fb(data=False))
    # statistics: whole blocks only, at least 4 of at least 16 samples
    for call in (be.rfi_stats, be.rfi_mask):
        with pytest.raises(ValueError, match="block 15 < 16"):
            call(_fb(), block=15)
        with pytest.raises(ValueError, match="at least 4"):
            call(_fb(n=4095), block=1024)
        with pytest.raises(ValueError, match="integers"):
            call(_fb(), block=100.5)
    assert be._rfi_stats_plan(_fb(n=4096 + 1000), 1024) == (1024, 4, 64, 5096)
    assert be._rfi_stats_plan(_fb(shard=(16, 48)), 1024) == (1024, 16, 32, 16384)
    # mask parameters
    for kw, word in ((dict(thresh=0), "thresh"), (dict(thresh=np.nan), "thresh"), (dict(chan_thresh=-1), "chan_thresh"),
                     (dict(chan_thresh=np.inf), "chan_thresh"), (dict(chan_window=4), "odd"), (dict(chan_window=0), "odd"),
                     (dict(chan_window=2.5), "integers"), (dict(chanfrac=1.5), "chanfrac"), (dict(intfrac=-0.1), "intfrac"),
                     (dict(zap_chans=[64]), "zap_chans"), (dict(zap_chans=[-1]), "zap_chans"),
                     (dict(zap_chans=[1.5]), "zap_chans"), (dict(zap_blocks=[16]), "zap_blocks"),
                     (dict(zap_blocks=[[1, 2]]), "zap_blocks")):
        with pytest.raises(ValueError, match=word):
            be.rfi_mask(_fb(), **kw)
    plan = be._rfi_mask_plan(_fb(), 1024, 5, 4, 17, 0.5, 0.25, (3, 5), [15])
    assert plan[:9] == (1024, 16, 64, 16384, 5.0, 4.0, 8, 0.5, 0.25)
    assert plan[9].tolist() == [3, 5] and plan[10].tolist() == [15]
    # the mask must fit the signal
    with pytest.raises(ValueError, match="RfiMask"):
        be.rfi_clean(_fb(), np.zeros((16, 64), dtype=bool))
    with pytest.raises(ValueError, match="channels"):
        be.rfi_clean(_fb(), _mask(C=32))
    with pytest.raises(ValueError, match="nsamp"):
        be.rfi_clean(_fb(), _mask(nsamp=16000))
    with pytest.raises(ValueError, match="block"):
        be.rfi_clean(_fb(), _mask(block=512))
    with pytest.raises(ValueError, match="block"):
        be.rfi_clean(_fb(), _mask(nb=15))
    with pytest.raises(ValueError, match="block"):
        be.rfi_clean(_fb(), _mask(block=0))
    # the zero-DM mean needs every channel; mask replacement on a shard is allowed
    part = _fb(shard=(16, 48))
    with pytest.raises(ValueError, match="whole band"):
        be.rfi_clean(part, _mask(C=32))
    assert be._rfi_clean_plan(part, _mask(C=32), False) == (32, 16384)
    assert be._rfi_clean_plan(_fb(shard=(0, 64)), _mask(), True) == (64, 16384)
    assert be._rfi_clean_plan(_fb(n=16384 + 1000), _mask(nsamp=17384), True) == (64, 17384)      # a ragged tail
    m = _mask()
    assert isinstance(m, RfiMask) and m.frac == 0.0 and m.zapped_chans().size == 0
    assert tuple(m.chan_frac.shape) == (64,) and tuple(m.block_frac.shape) == (16,)
    assert "16 blocks of 1024 samples x 64 channels" in repr(m)
    m.mask[:, 7] = True
    assert m.zapped_chans().tolist() == [7] and m.frac == 1.0 / 64 and torch.all(m.block_frac == 1.0 / 64)


def test_cabi_rejections():
    """NULL pointers, each out-of-range scalar and overlapping extents return PSS_EINVAL with the argument named
    and no device touched."""
    p = host_pointer()
    other = host_pointer()

    def at(q, nbytes):
        return ctypes.c_void_p(q.value + nbytes)
    # pss_rfi_clean(data, nchan, n, ld, mask, block, nblk, base, rgood, zero_dm, out, out_ld, zser, stream)
    good = dict(data=p, nchan=4, n=100, ld=100, mask=p, block=30, nblk=3, base=p, rgood=p, zero_dm=1, out=other,
                out_ld=100, zser=None)
    far = at(other, 1 << 20)                                  # (never dereferenced: the checks precede any launch)
    check_rejections(_lib.load().pss_rfi_clean, good,
                     ((dict(data=None), "data"), (dict(mask=None), "mask"), (dict(base=None), "base"),
                      (dict(out=None), "out"), (dict(rgood=None), "rgood"),
                      (dict(zero_dm=2), "zero_dm 2"), (dict(zero_dm=-1), "zero_dm -1"),
                      (dict(nchan=0), "nchan 0"), (dict(nchan=-3), "nchan -3"),
                      (dict(n=0, ld=0, out_ld=0), "n 0"), (dict(n=-5), "n -5"),
                      (dict(ld=99), "ld 99"), (dict(out_ld=99), "out_ld 99"),
                      (dict(block=0), "block 0"), (dict(block=-2), "block -2"),
                      (dict(nblk=0), "nblk 0"), (dict(nblk=-1), "nblk -1"),
                      (dict(nblk=5), "nblk 5"), (dict(block=50), "nblk 3"), (dict(block=1 << 62, nblk=2), "nblk 2"),
                      # partial overlap: shifted by a sample, by a row, another pitch from the same base
                      (dict(data=far, out=at(far, 4)), "overlap"), (dict(data=at(far, 400), out=far), "overlap"),
                      (dict(data=far, out=at(far, 4 * 399)), "overlap"), (dict(data=far, out=far, out_ld=104), "overlap"),
                      # the launch grid: ceil(n / 256) workgroups in 31 bits
                      # (in place: any two distinct extents of that length would overlap)
                      (dict(n=1 << 40, ld=1 << 40, out_ld=1 << 40, out=p), "workgroups")),
                     prefix="rfi_clean: ")
    from psrsigsim_amd import build
    with open(os.path.join(build.ROOT, "include", "pss_hip.h")) as f:
        names = f.read()
    assert "pss_rfi_clean" in names and "pss_rfi_clean" in _lib.EXPORTS and hasattr(_lib.load(), "pss_rfi_clean")
    assert len(_lib.EXPORTS["pss_rfi_clean"][1]) == 14 and "pss_rficlean.hip" in build.UNITS


def test_inject_rfi_index_checks():
    import torch
    from psrsigsim_amd.telescope import inject_rfi
    from psrsigsim_amd.telescope.rfi import inject_rfi as same
    assert inject_rfi is same
    stub = _fb(nchan=8, n=100)
    for kw, word in ((dict(tones=[(8, 1.0)]), "tone channel 8"), (dict(tones=[(-1, 1.0)]), "tone channel -1"),
                     (dict(tones=[(1.5, 1.0)]), "integers"),
                     (dict(bursts=[(8, 0, 10, 2.0)]), "burst channel 8"), (dict(bursts=[(0, 10, 10, 2.0)]), "burst samples"),
                     (dict(bursts=[(0, -1, 10, 2.0)]), "burst samples"), (dict(bursts=[(0, 90, 101, 2.0)]), "burst samples"),
                     (dict(impulses=[(96, 5, 1.0)]), "impulse samples"), (dict(impulses=[(-1, 5, 1.0)]), "impulse samples"),
                     (dict(impulses=[(0, 0, 1.0)]), "impulse samples"),
                     (dict(tones=[(0, 1.0)], impulses=[(100, 1, 1.0)]), "impulse samples")):   # nothing changed: stub untouched
        with pytest.raises(ValueError, match=word):
            inject_rfi(stub, **kw)
    with pytest.raises(ValueError, match="fold"):
        inject_rfi(_fb(fold=True))
    # plain torch: a host tensor stands in for the device buffer
    sig = _fb(nchan=8, n=100)
    sig._buf = torch.ones((8, 100), dtype=torch.float32)
    assert inject_rfi(sig, tones=[(2, 0.5)], bursts=[(3, 10, 20, 3.0)], impulses=[(50, 4, 20.0), (96, 4, 1.0)]) is sig
    want = np.ones((8, 100), dtype=np.float32)
    want[2] += 0.5
    want[3, 10:20] *= 3
    want[:, 50:54] += 20
    want[:, 96:100] += 1
    assert np.array_equal(sig._buf.numpy(), want)
