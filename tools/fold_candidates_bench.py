#!/usr/bin/env python
"""Time the candidate fold (pss_fold_series) next to its yardsticks, measured
in the same process, and print one JSON line (optionally also to --out).

    python tools/fold_candidates_bench.py [--nser 256] [--reps 7] [--pmin 64] [--pmax 16384] [--out FILE]

Series (float32 [nser][T], uniform random data, row stride T rounded up to 4
samples as Backend.dedisperse leaves it): the two products of
tools/dedisperse_bench.py taken as series,
  * search : nser x (2^20 - 1969) samples;
  * chan   : nser x (65536 - 24615) samples;
each folded with one output row per series, nbin = 64, nsub = 32 (L = T // 32),
phi0 = 0 and periods log-spaced from --pmin = 64 to --pmax = 16384 samples across
the rows (--pmin = --pmax gives every row the same period: how the kernel's time
depends on the length of a bin's run of samples, period / nbin).
Per shape:
  * kernel            : pss_fold_series, hits included;
  * torch_composition : what a user would otherwise write from the same
    definition -- phi = u * inc in wrapping int64 tensor arithmetic,
    bin = (((phi >> 32) & 0xFFFFFFFF) * nbin) >> 32, index_add_ of the samples
    into a float64 cube, a cast to float32 (and a bincount for the hits, not
    timed);
  * device_copy       : a plain device copy of the series' bytes.
The kernel and the composition must agree: the hits exactly, the sums within
2^-24 |ref| + n_b 2^-53 A_b (n_b the bin's hits, A_b its sum of |x|: the final
rounding plus the worst case of a float64 accumulation in any order) -- checked
here on every element (agrees_with_composition).
Then the stage as a whole: Backend.fold_candidates (sub-banding by
pss_dedisperse, statistics, the fold) of --ncand candidates at as many DMs
(0 .. 100 pc/cm^3, periods log-spaced from 65 to 16384 samples) on a --nchan x
2^--log2n signal at 64 us, next to Backend.dedisperse of the same
signal at the same DMs.
Times are device events around each call after a warm-up call; the figure is
the median of --reps calls (min and max are kept).  Needs the GPU: there is no
CPU path.
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
    ap.add_argument("--nser", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--nbin", type=int, default=64)
    ap.add_argument("--nsub", type=int, default=32)
    ap.add_argument("--pmin", type=float, default=64.0)
    ap.add_argument("--pmax", type=float, default=16384.0)
    ap.add_argument("--nchan", type=int, default=2048)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--ncand", type=int, default=16)
    ap.add_argument("--no-composition", action="store_true", help="time the kernel and the copy only")
    ap.add_argument("--no-api", action="store_true", help="skip Backend.fold_candidates")
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
    nser, nbin, nsub = args.nser, args.nbin, args.nsub

    timed = functools.partial(bench_util.timed, reps=args.reps)

    res = {"reps": args.reps, "device": torch.cuda.get_device_name(dev), "nbin": nbin, "nsub": nsub,
           "library": os.path.basename(_lib.LIB_PATH), "rows": []}
    periods = np.exp(np.linspace(np.log(args.pmin), np.log(args.pmax), nser))
    inc_py = [Backend._phase_step(p) for p in periods]
    inc_d = torch.from_numpy(np.array(inc_py, dtype=np.uint64).view(np.int64)).to(dev)
    src_d = torch.arange(nser, dtype=torch.int32, device=dev)
    for name, T in (("search", (1 << 20) - 1969), ("chan", 65536 - 24615)):
        ld = (T + 3) // 4 * 4
        Ls = T // nsub
        n = nsub * Ls
        x = torch.rand((nser, ld), dtype=torch.float32, device=dev)[:, :T]
        out = torch.empty((nser, nsub, nbin), dtype=torch.float32, device=dev)
        hits = torch.empty((nser, nsub, nbin), dtype=torch.int32, device=dev)

        def kern():
            _lib.check(L.pss_fold_series(x.data_ptr(), nser, T, ld, src_d.data_ptr(), inc_d.data_ptr(), None, nser,
                                         nsub, Ls, nbin, out.data_ptr(), hits.data_ptr(), st), "fold_series")

        e = {"shape": name, "series": nser, "samples": T, "L": Ls, "series_bytes": nser * T * 4,
             "period_samples": [round(float(periods[0]), 3), round(float(periods[-1]), 3)]}
        e["kernel"] = timed(kern)
        e["kernel"]["samples_per_s"] = round(nser * n / (e["kernel"]["ms"] * 1e-3), 1)
        e["kernel"]["series_GBps"] = round(e["series_bytes"] / (e["kernel"]["ms"] * 1e-3) / 1e9, 1)
        dst = torch.empty((nser, ld), dtype=torch.float32, device=dev)[:, :T]
        e["device_copy"] = timed(lambda: dst.copy_(x))
        e["device_copy"]["GBps"] = round(2 * e["series_bytes"] / (e["device_copy"]["ms"] * 1e-3) / 1e9, 1)
        e["kernel_over_copy"] = round(e["kernel"]["ms"] / e["device_copy"]["ms"], 2)
        del dst
        torch.cuda.empty_cache()
        if not args.no_composition:
            u = torch.arange(n, dtype=torch.int64, device=dev)
            base = (torch.arange(nser, dtype=torch.int64, device=dev) * (nsub * nbin))[:, None] + (u // Ls * nbin)[None, :]
            keep = {}

            def index():
                phi = u[None, :] * inc_d[:, None]                       # wraps: the phase mod 2^64
                return base + ((((phi >> 32) & 0xFFFFFFFF) * nbin) >> 32)

            def comp():
                idx = index().reshape(-1)
                acc = torch.zeros(nser * nsub * nbin, dtype=torch.float64, device=dev)
                acc.index_add_(0, idx, x[:, :n].reshape(-1).to(torch.float64))
                keep["sum"] = acc
                keep["out"] = acc.to(torch.float32)

            e["torch_composition"] = timed(comp)
            e["torch_over_kernel"] = round(e["torch_composition"]["ms"] / e["kernel"]["ms"], 2)
            e["kernel_beats_torch"] = bool(e["kernel"]["ms"] < e["torch_composition"]["ms"])
            idx = index().reshape(-1)
            cnt = torch.bincount(idx, minlength=nser * nsub * nbin)
            mag = torch.zeros(nser * nsub * nbin, dtype=torch.float64, device=dev)
            mag.index_add_(0, idx, x[:, :n].reshape(-1).to(torch.float64).abs())
            del idx
            want = keep["sum"]
            err = (out.reshape(-1).to(torch.float64) - want).abs()
            bound = 2.0 ** -24 * want.abs() + cnt.to(torch.float64) * 2.0 ** -53 * mag
            e["hits_equal_composition"] = bool(torch.equal(hits.reshape(-1).to(torch.int64), cnt))
            e["agrees_with_composition"] = bool((err <= bound).all().item()) and e["hits_equal_composition"]
            e["max_err_over_bound"] = float((err / bound.clamp_min(1e-300)).max().item())
            del u, base, keep, want, err, bound, cnt, mag
            torch.cuda.empty_cache()
        res["rows"].append(e)
        print(json.dumps(e), file=sys.stderr)
        del x, out, hits
        torch.cuda.empty_cache()

    if not args.no_api:
        # the stage as a whole next to Backend.dedisperse, same signal, same DMs
        C, N, K = args.nchan, 1 << args.log2n, args.ncand
        sig = FilterBankSignal(1400, 400, Nsubband=C, sample_rate=1000.0, fold=False)
        sig._samprate = make_quant(1.0 / 64.0, 'MHz')          # (set here: the constructor warns below Nyquist)
        sig._buf = torch.rand((C, N), dtype=torch.float32, device=dev)
        sig._ncols = sig._nsamp = N
        be = Backend(samprate=1.0 / 64.0, name="bench")
        dms = np.linspace(0.0, 100.0, K)
        per = np.exp(np.linspace(np.log(65.0), np.log(16384.0), K)) * 64e-6
        a = {"channels": C, "samples": N, "candidates": K, "unique_dms": K, "nband": 8, "nbin": nbin, "nsub": nsub}
        keep = {}

        def fold():
            keep["fc"] = be.fold_candidates(sig, dms=dms, periods=per, nbin=nbin, nsub=nsub, nband=8)

        a["fold_candidates"] = timed(fold)
        a["series_samples"] = keep["fc"].T
        a["dedisperse"] = timed(lambda: be.dedisperse(sig, dms))
        a["fold_over_dedisperse"] = round(a["fold_candidates"]["ms"] / a["dedisperse"]["ms"], 2)
        res["api"] = a

    bench_util.emit(res, args.out)


if __name__ == "__main__":
    main()
