#!/usr/bin/env python
"""Time the incoherent dedispersion (pss_dedisperse) next to two yardsticks
measured in the same process, and print one JSON line (optionally also to
--out).

    python tools/dedisperse_bench.py [--nchan 2048] [--log2n 20] [--ndm 256] [--reps 7] [--out FILE]

Shapes (float32 [chan][time], 1200-1600 MHz, trial DMs 0 .. 100 pc/cm^3, the
delays of Backend.dedisperse_delays):
  * search : nchan x 2^log2n samples at 64 us, ndm trials;
  * chan   : the channeliser's product of 2^28 voltages at C = 2048 -- 2048
    channels x 65536 samples at 800 MHz / 4096 = 195.3 kHz, ndm trials.
Per shape:
  * kernel            : pss_dedisperse as Backend.dedisperse calls it (aligned
    data, out_ld = T rounded up to 4 samples);
  * torch_composition : what a user would otherwise write -- per trial the
    index t + d[j][c], torch.gather of the [C, T] shifted rows, sum(0);
  * device_copy       : a plain device copy of the input bytes.
Times are device events around each call after a warm-up call; the figure is
the median of --reps calls (min and max are kept).  additions = C * T * ndm, the
adds of the direct sum.  Needs the GPU: there is no CPU path.
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
    ap.add_argument("--ndm", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from psrsigsim_amd import _lib
    from psrsigsim_amd._units import make_quant
    from psrsigsim_amd.signal import FilterBankSignal
    from psrsigsim_amd.telescope import Backend
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream

    timed = functools.partial(bench_util.timed, reps=args.reps)

    res = {"reps": args.reps, "device": torch.cuda.get_device_name(dev), "shapes": []}
    dms = np.linspace(0.0, 100.0, args.ndm)
    shapes = [("search", args.nchan, 1 << args.log2n, 1.0 / 64.0),
              ("chan", 2048, (1 << 28) // 4096, 800.0 / 4096.0)]
    for name, C, N, rate in shapes:
        sig = FilterBankSignal(1400, 400, Nsubband=C, sample_rate=1000.0, fold=False)
        sig._samprate = make_quant(rate, 'MHz')                # (set here: the constructor warns below Nyquist)
        delays = Backend.dedisperse_delays(sig, dms)
        md = int(delays.max())
        T = N - md
        Tp = (T + 3) // 4 * 4
        ndm = delays.shape[0]
        x = torch.rand((C, N), dtype=torch.float32, device=dev)
        tab = torch.from_numpy(delays).to(dev)
        out = torch.empty((ndm, Tp), dtype=torch.float32, device=dev)

        def kern():
            _lib.check(L.pss_dedisperse(x.data_ptr(), C, N, N, tab.data_ptr(), ndm, md, out.data_ptr(), Tp, st),
                       "dedisperse")

        adds = C * T * ndm
        e = {"shape": name, "nchan": C, "nsamp": N, "ndm": ndm, "samprate_MHz": rate, "max_delay": md,
             "out_samples": T, "additions": adds,
             "max_spread_in_8_trials": int(max(np.ptp(delays[g:g + 8], axis=0).max() for g in range(0, ndm, 8)))}
        dst = torch.empty_like(x)
        e["device_copy"] = timed(lambda: dst.copy_(x))
        e["device_copy"]["GBps"] = round(2 * C * N * 4 / (e["device_copy"]["ms"] * 1e-3) / 1e9, 1)
        del dst
        torch.cuda.empty_cache()
        e["kernel"] = timed(kern)
        e["kernel"]["additions_per_s"] = round(adds / (e["kernel"]["ms"] * 1e-3), 1)
        e["kernel_over_copy"] = round(e["kernel"]["ms"] / e["device_copy"]["ms"], 2)

        t = torch.arange(T, device=dev, dtype=torch.int64)
        tab64 = tab.to(torch.int64)
        comp_out = torch.empty((ndm, T), dtype=torch.float32, device=dev)

        def comp():
            for j in range(ndm):
                idx = t[None, :] + tab64[j][:, None]
                comp_out[j] = torch.gather(x, 1, idx).sum(0)
        e["torch_composition"] = timed(comp)
        e["torch_composition"]["additions_per_s"] = round(adds / (e["torch_composition"]["ms"] * 1e-3), 1)
        e["torch_over_kernel"] = round(e["torch_composition"]["ms"] / e["kernel"]["ms"], 2)
        e["kernel_beats_torch"] = bool(e["kernel"]["ms"] < e["torch_composition"]["ms"])
        # the two sum in different orders: a float32 sum of C terms in [0, 1)
        e["max_rel_diff_vs_torch"] = float(((out[:, :T] - comp_out).abs().max() / comp_out.abs().max()).item())
        res["shapes"].append(e)
        del x, out, comp_out, t, tab64
        torch.cuda.empty_cache()
    bench_util.emit(res, args.out)


if __name__ == "__main__":
    main()
