#!/usr/bin/env python
"""Time the search-mode output kernels (pss_chan_stats, pss_quantize_tmajor)
at a product geometry, next to a plain device copy of the same grid measured
in the same process, and print one JSON line (optionally also to --out).

    python tools/search_out_bench.py [--nchan 2048] [--log2n 22] [--nsblk 4096]
                                     [--nbits 8] [--reps 7] [--out FILE]

Times are device events around each launch after a warm-up launch; the
figure per kernel is the median of --reps launches (min and max are kept).
Bytes are algorithmic, computed from the shapes: the stats pass reads the
grid once; the quantiser reads it once and writes nchan*nbits/8 bytes per
time sample; the copy reads and writes it once.  Fractions are of the 8 TB/s
HBM peak bench.py uses.  The grid is filled with the library's own chi2(1)
draws.  Needs the GPU: there is no CPU path.
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
    ap.add_argument("--nchan", type=int, default=2048)
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--nsblk", type=int, default=4096)
    ap.add_argument("--nbits", type=int, default=8, choices=(8, 4, 2))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from psrsigsim_amd import _lib
    L = _lib.lib()
    nchan, nsamp, nsblk, nbits = args.nchan, 1 << args.log2n, args.nsblk, args.nbits
    nrows = nsamp // nsblk
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream

    timed = functools.partial(bench_util.timed, reps=args.reps)

    def rate(entry, nbytes):
        entry["alg_bytes"] = nbytes
        entry["GBps"] = round(nbytes / (entry["ms"] * 1e-3) / 1e9, 1)
        entry["hbm_frac"] = round(entry["GBps"] / HBM_PEAK_GBS, 4)
        return entry

    data = torch.empty((nchan, nsamp), dtype=torch.float32, device=dev)
    _lib.check(L.pss_chi2_fill(data.data_ptr(), nchan, 0, nsamp, 1.0, 12345, 1, _lib.P_TEST, st), "chi2_fill")
    grid_bytes = nchan * nsamp * 4

    dst = torch.empty_like(data)
    res = {"nchan": nchan, "nsamp": nsamp, "nsblk": nsblk, "nbits": nbits, "nrows": nrows, "reps": args.reps,
           "device": torch.cuda.get_device_name(dev)}
    res["device_copy"] = rate(timed(lambda: dst.copy_(data)), 2 * grid_bytes)
    del dst
    torch.cuda.empty_cache()

    mn = torch.empty((nrows, nchan), dtype=torch.float32, device=dev)
    mx = torch.empty_like(mn)
    s1 = torch.empty((nrows, nchan), dtype=torch.float64, device=dev)
    s2 = torch.empty_like(s1)

    def stats():
        _lib.check(L.pss_chan_stats(data.data_ptr(), nchan, nsamp, nsblk, nrows, mn.data_ptr(), mx.data_ptr(),
                                    s1.data_ptr(), s2.data_ptr(), st), "chan_stats")
    res["chan_stats"] = rate(timed(stats), grid_bytes)

    scl = ((mx - mn).double() / ((1 << nbits) - 1)).float()
    out_bytes = nrows * nsblk * nchan * nbits // 8
    out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)

    def quant():
        _lib.check(L.pss_quantize_tmajor(data.data_ptr(), nchan, nsamp, nsblk, nrows, scl.data_ptr(), mn.data_ptr(),
                                         nbits, out.data_ptr(), st), "quantize_tmajor")
    res["quantize_tmajor"] = rate(timed(quant), grid_bytes + out_bytes)
    for k in ("chan_stats", "quantize_tmajor"):
        res[k]["vs_copy_rate"] = round(res[k]["GBps"] / res["device_copy"]["GBps"], 3)
    bench_util.emit(res, args.out)


if __name__ == "__main__":
    main()
