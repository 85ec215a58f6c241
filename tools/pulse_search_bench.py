#!/usr/bin/env python
"""Time the boxcar single-pulse search (pss_boxcar_search) next to its
yardsticks, measured in the same process, and print one JSON line (optionally
also to --out).

    python tools/pulse_search_bench.py [--ndm 256] [--reps 7] [--out FILE]

Planes (float32 [ndm][T], uniform random data, row stride T rounded up to 4
samples as Backend.dedisperse leaves it): the two products of
tools/dedisperse_bench.py,
  * search : ndm x (2^20 - 1969) samples;
  * chan   : ndm x (65536 - 24615) samples;
each at nwidths 8 and 13, cell 32.  Per row:
  * kernel            : pss_boxcar_search as Backend.boxcar_snr calls it (the
    statistics of Backend._trial_stats, out_ld = cells rounded up to 16);
  * device_copy       : a plain device copy of the plane's bytes;
  * torch_composition : what a user would otherwise write -- the same doubling
    with slices per level, max_pool1d(cell, return_indices=True) per width and
    a running maximum;
  * statistics        : Backend._trial_stats alone (pss_chan_stats, the block
    medians in torch float64).
Times are device events around each call after a warm-up call; the figure is
the median of --reps calls (min and max are kept).  The composition performs
the kernel's float32 operations in the kernel's order, so the two S/N maps
must agree bit for bit (snr_equals_composition).  dedisperse_ms is read from
the committed measurement of pss_dedisperse on the same shape
(profiles/dedisperse/dedisperse_bench.json), when that file is there.  Needs
the GPU: there is no CPU path.
"""
import argparse
import functools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench_util  # noqa: E402  (tools/, next to this file)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndm", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cell", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import torch.nn.functional as F
    from psrsigsim_amd import _lib
    from psrsigsim_amd.telescope import Backend
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    cell, ndm = args.cell, args.ndm

    timed = functools.partial(bench_util.timed, reps=args.reps)

    dd = {}
    try:
        with open(os.path.join(ROOT, "profiles", "dedisperse", "dedisperse_bench.json")) as f:
            dd = {s["shape"]: s["kernel"]["ms"] for s in json.load(f)["shapes"] if s["ndm"] == ndm}
    except (OSError, ValueError, KeyError):
        pass

    res = {"reps": args.reps, "device": torch.cuda.get_device_name(dev), "cell": cell, "rows": []}
    for name, T in (("search", (1 << 20) - 1969), ("chan", 65536 - 24615)):
        ld = (T + 3) // 4 * 4
        x = torch.rand((ndm, ld), dtype=torch.float32, device=dev)[:, :T]
        nq = (T + cell - 1) // cell
        out_ld = (nq + 15) // 16 * 16
        snr = torch.empty((ndm, out_ld), dtype=torch.float32, device=dev)
        code = torch.empty((ndm, out_ld), dtype=torch.int32, device=dev)
        stats = timed(lambda: Backend._trial_stats(x, ld, 1024))
        mean, var = Backend._trial_stats(x, ld, 1024)
        mean32 = mean.to(torch.float32)
        rstd32 = (1.0 / torch.sqrt(var)).to(torch.float32)
        dst = torch.empty((ndm, ld), dtype=torch.float32, device=dev)
        copy = timed(lambda: dst.copy_(x.as_strided((ndm, ld), (ld, 1))))
        copy["GBps"] = round(2 * ndm * ld * 4 / (copy["ms"] * 1e-3) / 1e9, 1)
        del dst
        torch.cuda.empty_cache()
        for nw in (8, 13):
            def kern():
                _lib.check(L.pss_boxcar_search(x.data_ptr(), ndm, T, ld, mean32.data_ptr(), rstd32.data_ptr(), nw,
                                               cell, snr.data_ptr(), code.data_ptr(), out_ld, st), "boxcar_search")

            a = torch.tensor([2.0 ** -((k + 1) // 2) * (np.float32(np.sqrt(2.0)) if k & 1 else 1.0)
                              for k in range(nw)], dtype=torch.float32, device=dev)
            c = a[None, :] * rstd32[:, None]                       # c[j][k], one rounded product
            best = torch.empty((ndm, nq), dtype=torch.float32, device=dev)
            bcode = torch.empty((ndm, nq), dtype=torch.int64, device=dev)

            def comp():
                best.fill_(float("-inf"))
                bcode.zero_()
                S = x - mean32[:, None]
                for k in range(nw):
                    h = 1 << k
                    if h > T:
                        break
                    z = S * c[:, k, None]
                    v, i = F.max_pool1d(z[None], cell, stride=cell, ceil_mode=True, return_indices=True)
                    v, i = v[0], i[0]
                    n = v.shape[1]
                    upd = v > best[:, :n]
                    best[:, :n] = torch.where(upd, v, best[:, :n])
                    bcode[:, :n] = torch.where(upd, (k << 16) | (i % cell), bcode[:, :n])
                    if k + 1 < nw and 2 * h <= T:
                        S = S[:, :-h] + S[:, h:]

            e = {"shape": name, "ndm": ndm, "samples": T, "nwidths": nw, "cells": nq,
                 "plane_bytes": ndm * T * 4, "boxes": ndm * sum(max(T - (1 << k) + 1, 0) for k in range(nw))}
            e["kernel"] = timed(kern)
            e["kernel"]["boxes_per_s"] = round(e["boxes"] / (e["kernel"]["ms"] * 1e-3), 1)
            e["kernel"]["plane_GBps"] = round(e["plane_bytes"] / (e["kernel"]["ms"] * 1e-3) / 1e9, 1)
            e["device_copy"] = copy
            e["statistics"] = stats
            e["kernel_over_copy"] = round(e["kernel"]["ms"] / copy["ms"], 2)
            if name in dd:
                e["dedisperse_ms"] = dd[name]
                e["kernel_over_dedisperse"] = round(e["kernel"]["ms"] / dd[name], 4)
            e["torch_composition"] = timed(comp)
            e["torch_over_kernel"] = round(e["torch_composition"]["ms"] / e["kernel"]["ms"], 2)
            e["kernel_beats_torch"] = bool(e["kernel"]["ms"] < e["torch_composition"]["ms"])
            ks = snr[:, :nq]
            e["snr_equals_composition"] = bool(torch.equal(ks.view(torch.int32), best.view(torch.int32)))
            e["code_equals_composition"] = bool(torch.equal(code[:, :nq].to(torch.int64), bcode))
            e["max_snr"] = float(ks.max().item())
            res["rows"].append(e)
            del best, bcode
            torch.cuda.empty_cache()
        del x, snr, code
        torch.cuda.empty_cache()
    bench_util.emit(res, args.out)


if __name__ == "__main__":
    main()
