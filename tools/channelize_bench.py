#!/usr/bin/env python
"""Time the baseband channeliser (pss_channelize) at product shapes, next to
two yardsticks measured in the same process, and print one JSON line
(optionally also to --out).

    python tools/channelize_bench.py [--log2n 28] [--npol 2] [--reps 7] [--out FILE]

Shapes: npol x 2^log2n voltages, C in {64, 2048, 4096}, ntap in {1, 4},
tscrunch 1.  Per shape:
  * kernel            : as Backend.channelize calls it (aligned x, out_ld = S
    rounded up to 4 samples);
  * kernel_out_ld_S   : the same with out_ld = S, where S is no multiple of 4
    (the register-accumulator kernels then store dwords);
  * kernel_elem_loads (ntap = 1): x with a row stride of n + 1, so the loads
    are dwords -- the cost of a misaligned input;
  * torch_composition (ntap = 1): what a user would otherwise write --
    torch.fft.rfft of the [-1, L] view, abs()**2, the polarisation sum, the
    1/L scale and a transpose to [C][S] contiguous.
Also device_copy (a plain device copy of the input bytes) and normal_add
(pss_normal_add over the input: 4 B read + 4 B written per sample).
Times are device events around each call after a warm-up call; the figure is
the median of --reps calls (min and max are kept).  Bytes are algorithmic: the
kernel reads the voltages once and writes the [C][S] powers once.  Needs the
GPU: there is no CPU path.
"""
import argparse
import functools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_util  # noqa: E402  (tools/, next to this file)

HBM_PEAK_GBS = 8000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--npol", type=int, default=2, choices=(1, 2))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from psrsigsim_amd import _lib
    from psrsigsim_amd.telescope import Backend
    L = _lib.lib()
    npol, n = args.npol, 1 << args.log2n
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream

    timed = functools.partial(bench_util.timed, reps=args.reps)

    def rate(entry, nbytes):
        entry["alg_bytes"] = nbytes
        entry["GBps"] = round(nbytes / (entry["ms"] * 1e-3) / 1e9, 1)
        entry["hbm_frac"] = round(entry["GBps"] / HBM_PEAK_GBS, 4)
        return entry

    x = torch.zeros((npol, n), dtype=torch.float32, device=dev)
    _lib.check(L.pss_normal_add(x.data_ptr(), npol, n, n, 1.0, 12345, 1, st), "normal_add")
    in_bytes = npol * n * 4
    res = {"npol": npol, "nsamp": n, "reps": args.reps, "device": torch.cuda.get_device_name(dev), "shapes": []}
    dst = torch.empty_like(x)
    res["device_copy"] = rate(timed(lambda: dst.copy_(x)), 2 * in_bytes)
    del dst
    torch.cuda.empty_cache()

    def noise():
        _lib.check(L.pss_normal_add(x.data_ptr(), npol, n, n, 1e-3, 12345, 2, st), "normal_add")
    res["normal_add"] = rate(timed(noise), 2 * in_bytes)
    res["normal_add"]["vs_copy_rate"] = round(res["normal_add"]["GBps"] / res["device_copy"]["GBps"], 3)

    # the same voltages at a row stride of n + 1: no 16-B loads
    flat = torch.empty(npol * (n + 1), dtype=torch.float32, device=dev)
    xu = flat.as_strided((npol, n), (n + 1, 1))
    xu.copy_(x)

    for C in (64, 2048, 4096):
        Lf = 2 * C
        for T in (1, 4):
            S = n // Lf - T + 1
            Sp = (S + 3) // 4 * 4
            h = torch.from_numpy(Backend.pfb_coefficients(C, T).astype(np.float32)).to(dev)
            out = torch.empty(C * Sp, dtype=torch.float32, device=dev)

            def kern(xp=x.data_ptr(), ld=n, old=Sp):
                _lib.check(L.pss_channelize(xp, npol, n, ld, h.data_ptr(), C, T, 1, out.data_ptr(), old, st),
                           "channelize")

            def entry(fn):
                k = rate(timed(fn), in_bytes + C * S * 4)
                # the copy moves 2 x in_bytes; the kernel's rate over its own bytes against that
                k["vs_copy_rate"] = round(k["GBps"] / res["device_copy"]["GBps"], 3)
                return k
            e = {"nchan": C, "ntap": T, "tscrunch": 1, "nspectra": S, "out_ld_multiple_of_4": S % 4 == 0}
            if Sp != S:
                e["kernel_out_ld_S"] = entry(lambda: kern(old=S))
            if T == 1:
                e["kernel_elem_loads"] = entry(lambda: kern(xp=xu.data_ptr(), ld=n + 1))
            e["kernel"] = entry(kern)                 # last: `out` holds its [C][Sp] result
            if T == 1:
                def comp():
                    X = torch.fft.rfft(x.view(npol, -1, Lf), dim=-1)[..., :C]
                    return ((X.abs() ** 2).sum(dim=0) * (1.0 / Lf)).t().contiguous()
                e["torch_composition"] = timed(comp)
                e["torch_over_kernel"] = round(e["torch_composition"]["ms"] / e["kernel"]["ms"], 2)
                ref = comp()
                got = out.view(C, Sp)[:, :S]
                e["max_rel_diff_vs_torch"] = float(((got - ref).abs().max() / ref.abs().max()).item())
                del ref, got
            res["shapes"].append(e)
            del out
            torch.cuda.empty_cache()
    bench_util.emit(res, args.out)


if __name__ == "__main__":
    main()
