#!/usr/bin/env python
"""Time the RFI cleaner (pss_rfi_clean) next to two yardsticks measured in the
same process, and the mask's statistics and rules, and print one JSON line
(optionally also to --out).

    python tools/rfi_bench.py [--nchan 2048] [--log2n 20] [--block 1024] [--reps 7] [--out FILE]

Shapes (float32 [chan][time], the two of tools/dedisperse_bench.py): nchan x
2^log2n samples ("search") and 2048 x 65536 ("chan", the channeliser's
product).  The mask flags a random 2 % of the (block, channel) cells and 8 whole
channels.  Per shape:
  * kernel            : pss_rfi_clean with zero_dm 0 and 1, out of place (rows
    on the 16-B grid) and in place;
  * torch_composition : what a user would otherwise write for zero_dm = 1 --
    where(good, x - base, 0), sum(0), times rgood, where(good, x - z, base) --
    with the mask already expanded to samples (not timed);
  * device_copy       : a plain device copy of the input bytes;
  * rfi_stats, rfi_mask : Backend.rfi_stats alone and the whole Backend.rfi_mask
    (statistics and rules).
Times are device events around each call after a warm-up call; the figure is
the median of --reps calls (min and max are kept).  bytes_per_sample is the
model traffic of a call (zero_dm out of place or in place: two reads and a
write, 12 B; zero_dm = 0 out of place: 8 B; in place: the flagged cells only)
and GBps that traffic over the time.  Needs the GPU: there is no CPU path.
"""
import argparse
import functools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_util  # noqa: E402  (tools/, next to this file)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nchan", type=int, default=2048)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--block", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from psrsigsim_amd import _lib
    from psrsigsim_amd._units import make_quant
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.telescope import Backend, RfiMask
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    be = Backend(samprate=0.01, name="B")
    timed = functools.partial(bench_util.timed, reps=args.reps)
    block = args.block

    res = {"reps": args.reps, "device": torch.cuda.get_device_name(dev), "block": block, "tile": 256,
           "waves_per_workgroup": 8, "shapes": []}
    for name, C, N in (("search", args.nchan, 1 << args.log2n), ("chan", 2048, (1 << 28) // 4096)):
        nb = N // block
        rng = np.random.default_rng(1)
        m = rng.random((nb, C)) < 0.02
        m[:, rng.choice(C, size=8, replace=False)] = True
        mask = torch.from_numpy(m).to(dev)
        x = torch.rand((C, N), dtype=torch.float32, device=dev)
        base = torch.full((C,), 0.5, dtype=torch.float32, device=dev)
        good = (C - mask.sum(dim=1)).to(torch.float64)
        rgood = torch.where(good > 0, 1.0 / torch.clamp(good, min=1.0), torch.zeros_like(good)).to(torch.float32)
        mbytes = mask.to(torch.uint8).contiguous()
        out = torch.empty_like(x)
        zser = torch.empty((N,), dtype=torch.float32, device=dev)
        e = {"shape": name, "nchan": C, "nsamp": N, "nblk": nb, "flagged_frac": round(float(m.mean()), 5)}

        dst = torch.empty_like(x)
        e["device_copy"] = timed(lambda: dst.copy_(x))
        e["device_copy"]["GBps"] = round(2 * C * N * 4 / (e["device_copy"]["ms"] * 1e-3) / 1e9, 1)
        del dst
        torch.cuda.empty_cache()

        def kern(zero_dm, inplace):
            o = x if inplace else out
            _lib.check(L.pss_rfi_clean(x.data_ptr(), C, N, N, mbytes.data_ptr(), block, nb, base.data_ptr(),
                                       rgood.data_ptr() if zero_dm else None, zero_dm, o.data_ptr(), N,
                                       zser.data_ptr() if zero_dm else None, st), "rfi_clean")

        # the composition first: the in-place kernel runs change x
        good_s = ~mask.repeat_interleave(block, dim=0)
        if N > nb * block:
            good_s = torch.cat((good_s, good_s[-1:].expand(N - nb * block, C)))
        good_s = good_s.T.contiguous()                           # [C][N]
        rg_s = rgood.repeat_interleave(block)
        if N > nb * block:
            rg_s = torch.cat((rg_s, rg_s[-1:].expand(N - nb * block)))
        zero = torch.zeros((), dtype=torch.float32, device=dev)
        keep = {}

        def comp():
            z = torch.where(good_s, x - base[:, None], zero).sum(0) * rg_s
            keep["out"] = torch.where(good_s, x - z[None, :], base[:, None])
            keep["z"] = z
        e["torch_composition"] = timed(comp)
        kern(1, False)
        torch.cuda.synchronize()
        # the two sum in different orders: a float32 sum of about C terms in [-0.5, 0.5)
        e["max_abs_diff_vs_torch"] = float((out - keep["out"]).abs().max().item())
        keep.clear()
        del good_s, rg_s
        torch.cuda.empty_cache()

        flagged = float(m.mean())
        for zero_dm, inplace, bps in ((1, False, 12.0), (1, True, 12.0), (0, False, 8.0), (0, True, 4.0 * flagged)):
            k = "kernel_zdm%d_%s" % (zero_dm, "inplace" if inplace else "outofplace")
            e[k] = timed(functools.partial(kern, zero_dm, inplace))
            e[k]["bytes_per_sample"] = round(bps, 3)
            e[k]["GBps"] = round(bps * C * N / (e[k]["ms"] * 1e-3) / 1e9, 1)
            e[k]["over_copy"] = round(e[k]["ms"] / e["device_copy"]["ms"], 3)
        e["torch_over_kernel"] = round(e["torch_composition"]["ms"] / e["kernel_zdm1_outofplace"]["ms"], 2)
        e["kernel_beats_torch"] = bool(e["kernel_zdm1_outofplace"]["ms"] < e["torch_composition"]["ms"])

        sig = FilterBankSignal(1400, 400, Nsubband=C, sample_rate=1000.0, fold=False)
        sig._samprate = make_quant(0.01, 'MHz')                  # (set here: the constructor warns below Nyquist)
        sig._buf, sig._ncols, sig._nsamp = x, N, N
        e["rfi_stats"] = timed(lambda: be.rfi_stats(sig, block))
        e["rfi_mask"] = timed(lambda: be.rfi_mask(sig, block))
        assert isinstance(be.rfi_mask(sig, block), RfiMask)
        res["shapes"].append(e)
        del x, out, zser, mask, mbytes, sig
        torch.cuda.empty_cache()
    bench_util.emit(res, args.out)


if __name__ == "__main__":
    main()
