#!/usr/bin/env python
"""Time the acceleration resampler (pss_accel_resample) next to its yardsticks,
measured in the same process, and print one JSON line (optionally also to
--out; profiles/accel_search/accel_bench.json is such a run).

    python tools/accel_bench.py [--nser 32] [--nacc 8] [--reps 7] [--out FILE]

Series (float32 [nser][T], normal random data, row stride T rounded up to 4
samples as Backend.dedisperse leaves it) at the lengths of
tools/dedisperse_bench.py's two products,
  * search : (2^20 - 1969) samples;
  * chan   : (65536 - 24615) samples;
each resampled for nacc accelerations whose mid-observation shifts are spread
evenly over +-64 samples -- rows series-major, the acceleration fastest, as
Backend.accel_snr lays them out, the float32 mean subtracted.  Per shape:
  * kernel            : pss_accel_resample of the product library (the
    staged route wherever its rule allows);
  * kernel_direct     : the same sources built with -DPSS_ACCEL_NO_STAGE=1, in
    which every row gathers from global memory -- the A/B behind the staged
    route (the variant library is built on first use; both are loaded in this
    process and must give the same bits, direct_equals_staged);
  * tiles             : the same sources built with -DPSS_ACCEL_RUNS=1 and 4
    (1024 and 4096 output times a workgroup, windows of twice that) next to
    the product's 2048 -- the A/B behind the tile; same bits;
  * kernel_dword_stores : the product kernel writing rows off the 16-B grid
    (out_ld = ld + 1), where it stores dwords instead of 16 B;
  * torch_composition : what a user would otherwise write -- torch.gather of
    the flattened series with the int64 index table computed on the host, then
    the subtraction.  Its output must equal the kernel's bit for bit
    (equals_composition; the tool asserts it);
  * device_copy       : a plain device copy of the output's bytes;
  * rfft, harmonic    : the transform (nfft = Backend.fft_length(T)) and the
    16-harmonic search of the same rows, the rest of an acceleration trial.
Times are device events around each call after a warm-up call; the figure is
the median of --reps calls (min and max are kept).  Needs the GPU: there is no
CPU path.
"""
import argparse
import functools
import os
import sys
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench_util  # noqa: E402  (tools/, next to this file)

VARIANT, VARIANT_FLAGS = "accel_nostage", ["-DPSS_ACCEL_NO_STAGE=1"]
TILES = (("1024", "accel_tb1024", ["-DPSS_ACCEL_RUNS=1"]), ("4096", "accel_tb4096", ["-DPSS_ACCEL_RUNS=4"]))


def shift_u64(np, T, K):
    """s(t) = (t (T - t) K + 2^63) >> 64 for t < T, exactly, in uint64 pieces
    (the 128-bit product by 32-bit halves)."""
    M = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    t = np.arange(T, dtype=np.uint64)
    u = t * (np.uint64(T) - t)                               # < 2^62
    uh, ul = u >> s32, u & M
    Kh, Kl = np.uint64(K >> 32), np.uint64(K & 0xFFFFFFFF)
    ll, lh, hl = ul * Kl, ul * Kh, uh * Kl
    mid = (ll >> s32) + (lh & M) + (hl & M)
    hi = uh * Kh + (lh >> s32) + (hl >> s32) + (mid >> s32)
    lo_top = (mid >> np.uint64(31)) & np.uint64(1)           # bit 63 of the low word
    return hi + lo_top


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nser", type=int, default=32)
    ap.add_argument("--nacc", type=int, default=8)
    ap.add_argument("--smax", type=float, default=64.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cell", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from psrsigsim_amd import _lib, build
    from psrsigsim_amd.telescope import Backend
    L = _lib.lib()
    Ld = _lib.load(build.build(variant=VARIANT, variant_flags=VARIANT_FLAGS, verbose=False))
    Lt = {tb: _lib.load(build.build(variant=v, variant_flags=fl, verbose=False)) for tb, v, fl in TILES}
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    nser, nacc, cell = args.nser, args.nacc, args.cell
    rows = nser * nacc

    timed = functools.partial(bench_util.timed, reps=args.reps)

    res = {"reps": args.reps, "device": torch.cuda.get_device_name(dev), "library": os.path.basename(_lib.LIB_PATH),
           "direct_library": "libpss_hip_%s.so (%s)" % (VARIANT, " ".join(VARIANT_FLAGS)), "rows": []}
    for name, T in (("search", (1 << 20) - 1969), ("chan", 65536 - 24615)):
        ld = (T + 3) // 4 * 4
        x = torch.randn((nser, ld), dtype=torch.float32, device=dev)
        smax = np.linspace(-args.smax, args.smax, nacc)
        kap = []
        for s in smax:
            q = Fraction(float(abs(s))) * 4 * (1 << 64) / (T * T) + Fraction(1, 2)
            kap.append((q.numerator // q.denominator) * (1 if s >= 0 else -1))
        src_d = torch.from_numpy(np.repeat(np.arange(nser, dtype=np.int32), nacc)).to(dev)
        kap_d = torch.from_numpy(np.tile(np.array(kap, dtype=np.int64), nser)).to(dev)
        mean, var = Backend._trial_stats(x[:, :T], ld, 1024)
        sub_d = mean.to(torch.float32).repeat_interleave(nacc)
        out_ld = ld
        out = torch.empty((rows, out_ld), dtype=torch.float32, device=dev)

        def kern(lib, o=None, o_ld=None):
            o, o_ld = (out, out_ld) if o is None else (o, o_ld)
            _lib.check(lib.pss_accel_resample(x.data_ptr(), nser, T, ld, src_d.data_ptr(), kap_d.data_ptr(),
                                              sub_d.data_ptr(), rows, T, o.data_ptr(), o_ld, st), "accel_resample")

        e = {"shape": name, "series": nser, "accelerations": nacc, "rows": rows, "samples": T,
             "smax": [round(float(s), 3) for s in smax], "output_bytes": rows * T * 4}
        e["kernel_direct"] = timed(lambda: kern(Ld))
        direct = out[:, :T].clone()
        out.zero_()
        e["kernel"] = timed(lambda: kern(L))
        e["direct_equals_staged"] = bool(torch.equal(direct.view(torch.int32), out[:, :T].view(torch.int32)))
        assert e["direct_equals_staged"]
        del direct
        # the tile: 1024 / 2048 (the product) / 4096 times a workgroup
        want = out[:, :T].clone()
        e["tiles"] = {"2048": dict(e["kernel"])}
        for tb, lib in Lt.items():
            out.zero_()
            e["tiles"][tb] = timed(lambda: kern(lib))
            e["tiles"][tb]["same_bits"] = bool(torch.equal(want.view(torch.int32), out[:, :T].view(torch.int32)))
            assert e["tiles"][tb]["same_bits"]
        # rows off the 16-B grid: dword stores
        off = torch.zeros((rows, ld + 1), dtype=torch.float32, device=dev)
        e["kernel_dword_stores"] = timed(lambda: kern(L, off, ld + 1))
        e["kernel_dword_stores"]["same_bits"] = bool(torch.equal(want.view(torch.int32), off[:, :T].view(torch.int32)))
        assert e["kernel_dword_stores"]["same_bits"]
        del off, want
        out.zero_()
        kern(L)
        e["kernel"]["output_GBps"] = round(e["output_bytes"] / (e["kernel"]["ms"] * 1e-3) / 1e9, 1)
        e["staged_over_direct"] = round(e["kernel"]["ms"] / e["kernel_direct"]["ms"], 3)
        # a device copy of the output's bytes
        dst = torch.empty((rows, T), dtype=torch.float32, device=dev)
        srcbuf = torch.empty_like(dst)
        e["device_copy"] = timed(lambda: dst.copy_(srcbuf))
        e["device_copy"]["GBps"] = round(2 * rows * T * 4 / (e["device_copy"]["ms"] * 1e-3) / 1e9, 1)
        del dst, srcbuf
        torch.cuda.empty_cache()
        # the composition: the index table from the host (Python integers), one gather, one subtraction
        t = np.arange(T, dtype=np.int64)
        idx = np.empty((nacc, T), dtype=np.int64)
        for a, k in enumerate(kap):
            K, sg = min(abs(k), (1 << 63) // T), (-1 if k < 0 else 1)
            idx[a] = np.clip(t + sg * shift_u64(np, T, K).astype(np.int64), 0, T - 1)
        flat = (torch.from_numpy(idx).to(dev)[None, :, :]
                + (torch.arange(nser, dtype=torch.int64, device=dev) * ld)[:, None, None]).reshape(rows, T)
        xf = x.view(-1)
        comp_out = torch.empty((rows, T), dtype=torch.float32, device=dev)

        def comp():
            torch.sub(torch.gather(xf, 0, flat.view(-1)).view(rows, T), sub_d[:, None], out=comp_out)

        e["torch_composition"] = timed(comp)
        e["index_table_bytes"] = rows * T * 8
        e["equals_composition"] = bool(torch.equal(comp_out.view(torch.int32), out[:, :T].view(torch.int32)))
        assert e["equals_composition"], "the kernel and the torch composition differ"
        e["torch_over_kernel"] = round(e["torch_composition"]["ms"] / e["kernel"]["ms"], 2)
        e["kernel_beats_torch"] = bool(e["kernel"]["ms"] < e["torch_composition"]["ms"])
        e["kernel_over_copy"] = round(e["kernel"]["ms"] / e["device_copy"]["ms"], 2)
        del flat, comp_out, idx
        torch.cuda.empty_cache()
        # the rest of an acceleration trial: the transform and the 16-harmonic search of the same rows
        nfft = Backend.fft_length(T)
        nbin = nfft // 2
        nq = (nbin + cell - 1) // cell
        q_ld = (nq + 15) // 16 * 16
        e["nfft"] = nfft
        e["rfft"] = timed(lambda: torch.fft.rfft(out[:, :nfft], n=nfft))
        spec = torch.fft.rfft(out[:, :nfft], n=nfft)
        scale32 = (1.0 / (var * nfft)).to(torch.float32).repeat_interleave(nacc)
        snr = torch.empty((rows, q_ld), dtype=torch.float32, device=dev)
        code = torch.empty((rows, q_ld), dtype=torch.int32, device=dev)
        work = torch.empty(rows * nbin, dtype=torch.float32, device=dev)
        e["harmonic"] = timed(lambda: _lib.check(L.pss_harmonic_search(
            spec.data_ptr(), rows, nbin, int(spec.shape[1]), scale32.data_ptr(), 5, 1, cell, snr.data_ptr(),
            code.data_ptr(), q_ld, work.data_ptr(), st), "harmonic_search"))
        rest = e["rfft"]["ms"] + e["harmonic"]["ms"]
        e["kernel_over_rfft_plus_harmonic"] = round(e["kernel"]["ms"] / rest, 3)
        e["kernel_share_of_trial"] = round(e["kernel"]["ms"] / (e["kernel"]["ms"] + rest), 3)
        res["rows"].append(e)
        del x, out, spec, snr, code, work
        torch.cuda.empty_cache()
    bench_util.emit(res, args.out)


if __name__ == "__main__":
    main()
