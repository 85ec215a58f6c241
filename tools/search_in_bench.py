#!/usr/bin/env python
"""Time the search-mode input kernel (pss_unpack_tmajor) at a product geometry
against the torch composition of the same result on the same device tensors,
next to a plain device copy of the float32 grid, and the whole loader
(load_search_signal) on a file in a temporary directory; print one JSON line
(optionally also to --out).

    python tools/search_in_bench.py [--nchan 2048] [--log2n 22] [--nsblk 4096]
                                    [--configs 8:1,4:1,2:1,8:2] [--reps 7]
                                    [--loader-reps 3] [--out FILE]

A config is NBITS:NPOL (NPOL 2 sums both polarisations).  All of them run in
one process.  Kernel and composition are timed in turn (bench_util.
timed_alternating: device events around each call after a warm-up call of
each), the figure is the median of --reps calls, min and max are kept: the
margin between the two is what those spreads show.  The composition is shift
and mask, cast, multiply-add, the sum of the polarisations, then a transpose
to contiguous -- torch operations only.  Bytes are algorithmic, computed from
the shapes: the kernel reads nsum * nbits / 8 bytes and writes 4 per output
sample; the copy reads and writes the grid once.  Fractions are of the 8 TB/s
HBM peak bench.py uses.

The loader is timed end to end (host clock around a call that ends in a
device synchronise) on an 8-bit file the package's own writer made from the
last config's grid, with two buffer pairs and with one, in turn,
--loader-reps times each (0: skip).  The file has just been written, so the
reads come from the page cache: the figure holds the copy into the pinned
buffer, the PCIe copy and the kernel, not a disk.  Needs the GPU: there is no
CPU path.
"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_util  # noqa: E402  (tools/, next to this file)

HBM_PEAK_GBS = 8000.0


def rate(entry, nbytes):
    entry["alg_bytes"] = nbytes
    entry["GBps"] = round(nbytes / (entry["ms"] * 1e-3) / 1e9, 1)
    entry["hbm_frac"] = round(entry["GBps"] / HBM_PEAK_GBS, 4)
    return entry


def compose(packed, scl, offs, nbits, nchan, npol, nsum, nsblk, nrows):
    """The torch composition of pss_unpack_tmajor (zero_off 0, no weights, no flip)."""
    import torch
    per = 8 // nbits
    b = packed.view(nrows, nsblk, npol, nchan // per)
    s, o = scl.view(nrows, 1, npol, nchan), offs.view(nrows, 1, npol, nchan)
    x = None
    for p in range(nsum):
        c = b[:, :, p]
        if per > 1:
            c = torch.stack([(c >> (8 - nbits * (k + 1))) & ((1 << nbits) - 1) for k in range(per)], dim=-1)
            c = c.reshape(nrows, nsblk, nchan)
        v = torch.addcmul(o[:, :, p], c.to(torch.float32), s[:, :, p])
        x = v if x is None else x.add_(v)
    return x.reshape(nrows * nsblk, nchan).t().contiguous()


def time_loader(grid, nchan, nsamp, nsblk, reps):
    """load_search_signal on the writer's 8-bit file of ``grid``, two buffer
    pairs against one."""
    import numpy as np
    import torch
    from psrsigsim_amd.io import PSRFITS, psrfits
    from psrsigsim_amd.signal import FilterBankSignal

    class Source(object):
        name = "J0000+0000"
    sig = FilterBankSignal(1400.0, 400.0, Nsubband=nchan, fold=False, dtype=np.float32)
    sig._buf, sig._ncols, sig._nsamp = grid, nsamp, nsamp
    res = {}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "search_in_bench.fits")
        t0 = time.perf_counter()
        PSRFITS(path, obs_mode="SEARCH").save(sig, Source(), nbits=8, nsblk=nsblk)
        res["write_s"] = round(time.perf_counter() - t0, 3)
        res["file_bytes"] = os.path.getsize(path)
        times = {1: [], 2: []}
        for i in range(reps + 1):                    # the first round warms up
            for nbuf in (2, 1):
                psrfits._LOAD_BUFFERS = nbuf
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                loaded = psrfits.load_search_signal(path)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                del loaded
                if i:
                    times[nbuf].append(dt)
        psrfits._LOAD_BUFFERS = 2
    for nbuf, key in ((2, "double_buffer"), (1, "single_buffer")):
        t = sorted(times[nbuf])
        res[key] = {"s": round(t[len(t) // 2], 4), "min_s": round(t[0], 4), "max_s": round(t[-1], 4),
                    "file_GBps": round(res["file_bytes"] / t[len(t) // 2] / 1e9, 2)}
    res["reps"] = reps
    res["file_cache"] = "warm (the file was just written)"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nchan", type=int, default=2048)
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--nsblk", type=int, default=4096)
    ap.add_argument("--configs", default="8:1,4:1,2:1,8:2")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--loader-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from psrsigsim_amd import _lib
    L = _lib.lib()
    nchan, nsamp, nsblk = args.nchan, 1 << args.log2n, args.nsblk
    nrows = nsamp // nsblk
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    grid_bytes = nchan * nsamp * 4
    res = {"nchan": nchan, "nsamp": nsamp, "nsblk": nsblk, "nrows": nrows, "reps": args.reps,
           "device": torch.cuda.get_device_name(dev), "configs": []}
    out = torch.empty((nchan, nsamp), dtype=torch.float32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(12345)

    first = None
    for cfg in args.configs.split(","):
        nbits, npol = (int(v) for v in cfg.split(":"))
        nsum = min(npol, 2)
        in_bytes = nrows * nsblk * npol * nchan * nbits // 8
        packed = torch.randint(0, 256, (in_bytes,), dtype=torch.uint8, device=dev, generator=gen)
        scl = torch.rand((nrows, npol, nchan), device=dev, generator=gen) + 0.5
        offs = torch.randn((nrows, npol, nchan), device=dev, generator=gen)

        def unpack():
            _lib.check(L.pss_unpack_tmajor(packed.data_ptr(), nchan, npol, nsum, nsblk, nrows, scl.data_ptr(),
                                           offs.data_ptr(), None, 0.0, nbits, 0, out.data_ptr(), nsamp, st),
                       "unpack_tmajor")

        def torch_compose():
            compose(packed, scl, offs, nbits, nchan, npol, nsum, nsblk, nrows)

        entry = {"nbits": nbits, "npol": npol, "nsum": nsum}
        # the two results agree (a multiply-add may or may not be fused in torch: one float32 rounding)
        unpack()
        ref = compose(packed, scl, offs, nbits, nchan, npol, nsum, nsblk, nrows)
        entry["max_abs_diff_vs_torch"] = float((ref - out).abs().max())
        del ref
        torch.cuda.empty_cache()
        t = bench_util.timed_alternating({"unpack_tmajor": unpack, "torch_composition": torch_compose}, args.reps)
        alg = nrows * nsblk * nchan * (4 + nsum * nbits / 8.0)
        entry["unpack_tmajor"] = rate(t["unpack_tmajor"], int(alg))
        entry["torch_composition"] = t["torch_composition"]
        entry["torch_over_kernel"] = round(t["torch_composition"]["ms"] / t["unpack_tmajor"]["ms"], 2)
        entry["torch_min_over_kernel_max"] = round(t["torch_composition"]["min_ms"] / t["unpack_tmajor"]["max_ms"], 2)
        res["configs"].append(entry)
        if first is None:
            first = True
            dst = torch.empty_like(out)
            res["device_copy"] = rate(bench_util.timed(lambda: dst.copy_(out), args.reps), 2 * grid_bytes)
            del dst
        del packed, scl, offs
        torch.cuda.empty_cache()
    for entry in res["configs"]:
        # rates of algorithmic bytes: the kernel moves fewer than the copy's 8 per sample
        entry["unpack_tmajor"]["vs_copy_rate"] = round(entry["unpack_tmajor"]["GBps"] / res["device_copy"]["GBps"], 3)
        entry["unpack_tmajor"]["vs_copy_time"] = round(entry["unpack_tmajor"]["ms"] / res["device_copy"]["ms"], 3)
    if args.loader_reps > 0:
        # the last config's grid: the writer quantises it to 8 bits whatever made it
        res["loader"] = time_loader(out, nchan, nsamp, nsblk, args.loader_reps)
    bench_util.emit(res, args.out)


if __name__ == "__main__":
    main()
