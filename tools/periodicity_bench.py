#!/usr/bin/env python
"""Time the harmonic-sum periodicity search (pss_harmonic_search) next to its
yardsticks, measured in the same process, and print one JSON line (optionally
also to --out).

    python tools/periodicity_bench.py [--ndm 256] [--reps 7] [--out FILE]

Planes (float32 [ndm][T], uniform random data, row stride T rounded up to 4
samples as Backend.dedisperse leaves it): the two products of
tools/dedisperse_bench.py,
  * search : ndm x (2^20 - 1969) samples;
  * chan   : ndm x (65536 - 24615) samples;
each transformed at nfft = Backend.fft_length(T) and searched at nharm 1 and
16, cell 32, kmin 1.  Per row:
  * kernel            : pss_harmonic_search as Backend.harmonic_snr calls it
    (one chunk, scale from Backend._trial_stats, out_ld = cells rounded up to
    16): with the workspace of its power pass at 8 and 16 harmonics,
    without it below.  Both ways are timed at every row, in this process
    (kernel_direct, kernel_power_pass: the A/B behind that rule; --nharm 1 2
    4 8 16 shows the crossover), and must give the same bits
    (direct_equals_power_pass);
  * device_copy       : a plain device copy of the spectrum's bytes;
  * rfft              : the transform that makes the spectrum (mean
    subtraction included), as Backend.dm_spectrum runs it;
  * statistics        : Backend._trial_stats alone;
  * torch_composition : what a user would otherwise write -- the power, one
    index-gather and add per odd m, max_pool1d(cell, return_indices=True) per
    level and a running maximum.
Times are device events around each call after a warm-up call; the figure is
the median of --reps calls (min and max are kept).  The composition performs
the kernel's float32 operations in the kernel's order, so the two maps must
agree bit for bit (snr_equals_composition, code_equals_composition).  Needs
the GPU: there is no CPU path.
"""
import argparse
import functools
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
    ap.add_argument("--nharm", type=int, nargs="+", default=[1, 16], choices=[1, 2, 4, 8, 16])
    ap.add_argument("--no-composition", action="store_true", help="time the kernel and the copies only")
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

    res = {"reps": args.reps, "device": torch.cuda.get_device_name(dev), "cell": cell,
           "library": os.path.basename(_lib.LIB_PATH), "rows": []}
    for name, T in (("search", (1 << 20) - 1969), ("chan", 65536 - 24615)):
        ld = (T + 3) // 4 * 4
        x = torch.rand((ndm, ld), dtype=torch.float32, device=dev)[:, :T]
        nfft = Backend.fft_length(T)
        nbin = nfft // 2
        nq = (nbin + cell - 1) // cell
        out_ld = (nq + 15) // 16 * 16
        snr = torch.empty((ndm, out_ld), dtype=torch.float32, device=dev)
        code = torch.empty((ndm, out_ld), dtype=torch.int32, device=dev)
        stats = timed(lambda: Backend._trial_stats(x, ld, 1024))
        mean, var = Backend._trial_stats(x, ld, 1024)
        mean32 = mean.to(torch.float32)
        scale32 = (1.0 / (var * nfft)).to(torch.float32)
        fft = timed(lambda: Backend._spectrum_rows(x, mean32, 0, ndm, nfft, nfft))
        spec = Backend._spectrum_rows(x, mean32, 0, ndm, nfft, nfft)
        sld = int(spec.shape[1])
        dst = torch.empty_like(spec)
        copy = timed(lambda: dst.copy_(spec))
        copy["GBps"] = round(2 * ndm * sld * 8 / (copy["ms"] * 1e-3) / 1e9, 1)
        del dst
        torch.cuda.empty_cache()
        work = torch.empty(ndm * nbin, dtype=torch.float32, device=dev)
        for nharm in args.nharm:
            nl = nharm.bit_length()

            def kern(w=None):
                _lib.check(L.pss_harmonic_search(spec.data_ptr(), ndm, nbin, sld, scale32.data_ptr(), nl, 1, cell,
                                                 snr.data_ptr(), code.data_ptr(), out_ld,
                                                 None if w is None else w.data_ptr(), st), "harmonic_search")

            e = {"shape": name, "ndm": ndm, "samples": T, "nfft": nfft, "bins": nbin, "nharm": nharm, "cells": nq,
                 "spectrum_bytes": ndm * sld * 8, "terms": ndm * nbin * nharm}
            # both sources of the terms, same process: gathers from the spectrum, and the power pass
            e["kernel_direct"] = timed(kern)
            direct = (snr.clone(), code.clone())
            e["kernel_power_pass"] = timed(lambda: kern(work))
            e["direct_equals_power_pass"] = bool(torch.equal(direct[0].view(torch.int32)[:, :nq],
                                                             snr.view(torch.int32)[:, :nq])
                                                 and torch.equal(direct[1][:, :nq], code[:, :nq]))
            del direct
            # what Backend.harmonic_snr runs: the power pass at 8 and 16 harmonics
            e["kernel"] = dict(e["kernel_power_pass"] if nharm > 4 else e["kernel_direct"])
            e["kernel"]["terms_per_s"] = round(e["terms"] / (e["kernel"]["ms"] * 1e-3), 1)
            e["kernel"]["spectrum_GBps"] = round(e["spectrum_bytes"] / (e["kernel"]["ms"] * 1e-3) / 1e9, 1)
            e["device_copy"] = copy
            e["rfft"] = fft
            e["statistics"] = stats
            e["kernel_over_copy"] = round(e["kernel"]["ms"] / copy["ms"], 2)
            e["kernel_over_rfft"] = round(e["kernel"]["ms"] / fft["ms"], 3)
            ks = snr[:, :nq]
            e["max_snr"] = float(ks.max().item())
            if not args.no_composition:
                k = torch.arange(nbin, dtype=torch.int64, device=dev)
                a = [float(np.float32(2.0 ** -((l + 1) // 2) * (np.float32(np.sqrt(2.0)) if l & 1 else 1.0)))
                     for l in range(nl)]
                gather = {(l, m): (k * m + (1 << l) // 2) // (1 << l) for l in range(1, nl)
                          for m in range(1, 1 << l, 2)}
                valid = [((k + (1 << l) // 2) // (1 << l)) >= 1 for l in range(nl)]
                ninf = torch.tensor(float("-inf"), dtype=torch.float32, device=dev)
                best = torch.empty((ndm, nq), dtype=torch.float32, device=dev)
                bcode = torch.empty((ndm, nq), dtype=torch.int64, device=dev)
                sr = torch.view_as_real(spec)

                def comp():
                    best.fill_(float("-inf"))
                    bcode.zero_()
                    re, im = sr[:, :nbin, 0], sr[:, :nbin, 1]
                    P = (re * re + im * im) * scale32[:, None]       # (eager torch: three rounded operations)
                    H = P
                    for l in range(nl):
                        for m in range(1, 1 << l, 2):
                            H = H + P.index_select(1, gather[(l, m)])
                        z = torch.where(valid[l][None, :], (H - float(1 << l)) * a[l], ninf)
                        v, i = F.max_pool1d(z[None], cell, stride=cell, ceil_mode=True, return_indices=True)
                        v, i = v[0], i[0]
                        upd = v > best
                        best.copy_(torch.where(upd, v, best))
                        bcode.copy_(torch.where(upd, (l << 16) | (i % cell), bcode))

                e["torch_composition"] = timed(comp)
                e["torch_over_kernel"] = round(e["torch_composition"]["ms"] / e["kernel"]["ms"], 2)
                e["kernel_beats_torch"] = bool(e["kernel"]["ms"] < e["torch_composition"]["ms"])
                e["snr_equals_composition"] = bool(torch.equal(ks.view(torch.int32), best.view(torch.int32)))
                e["code_equals_composition"] = bool(torch.equal(
                    torch.where(ks == ninf, 0, code[:, :nq].to(torch.int64)), torch.where(best == ninf, 0, bcode)))
                del best, bcode, gather, valid
                torch.cuda.empty_cache()
            res["rows"].append(e)
        del x, snr, code, spec, work
        torch.cuda.empty_cache()
    bench_util.emit(res, args.out)


if __name__ == "__main__":
    main()
