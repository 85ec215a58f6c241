#!/usr/bin/env python
"""Time the template match (pss_toa_fit) next to its yardsticks, measured in
the same process, and print one JSON line (optionally also to --out;
profiles/toa/toa_bench.json is such a run).

    python tools/toa_bench.py [--nchan 2048] [--nsub 15] [--reps 7] [--out FILE]

Profiles: a three-component template shifted by a random phase per profile
under Gaussian noise (b / b_err about 100), float32 [nchan][nsub * nbin] -- the
layout of a fold-mode signal -- at 2048 bins (C4's own shape with 2048 channels
x 15 sub-integrations: the FFT path) and at 2000 bins (the direct path).  Per
shape:
  * toa_fit : the kernel of the product library with one template for all
    channels, and toa_fit_per_channel with a template per channel;
  * copy : a plain device copy of the same bytes (the kernel reads every
    profile once and writes 32 B a profile);
  * torch_coarse : what a user would otherwise write -- torch.fft.rfft, the
    cross-spectrum with the conjugate template, irfft and argmax.  That is the
    coarse stage alone: no refinement, no error bars, so it does less than the
    kernel.  Its maximum must be the grid point next to the kernel's tau.
Times are device events around each call after a warm-up call; the figure is
the median of --reps calls (min and max are kept).  Needs the GPU: there is no
CPU path.
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
    ap.add_argument("--nchan", type=int, default=2048)
    ap.add_argument("--nsub", type=int, default=15)
    ap.add_argument("--nbins", type=int, nargs="+", default=[2048, 2000])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from psrsigsim_amd import _lib
    from psrsigsim_amd.telescope import Backend
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    nchan, nsub = args.nchan, args.nsub
    timed = functools.partial(bench_util.timed, reps=args.reps)

    res = {"reps": args.reps, "device": torch.cuda.get_device_name(dev), "library": os.path.basename(_lib.LIB_PATH),
           "rows": []}
    for nbin in args.nbins:
        ph = np.arange(nbin) / nbin
        tm = sum(a * np.exp((np.cos(2 * np.pi * (ph - c)) - 1) / (2 * np.pi * w) ** 2)
                 for c, w, a in ((0.30, 0.03, 1.0), (0.36, 0.05, 0.45), (0.22, 0.08, 0.2)))
        one = Backend.toa_template(tm, nbin)
        per = Backend.toa_template(tm[None, :] * (1.0 + np.arange(nchan)[:, None] / nchan), nbin)
        K = one.K
        # the profiles on the device: the shift theorem on the template's spectrum
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        tau = torch.rand((nchan, nsub, 1), generator=g, device=dev, dtype=torch.float64) - 0.5
        S = torch.from_numpy(np.fft.rfft(tm)).to(dev)
        k = torch.arange(S.shape[0], device=dev, dtype=torch.float64)
        prof = torch.fft.irfft(S * torch.exp(-2j * np.pi * k * tau), n=nbin)
        sigma = float(np.sqrt(2 * one.S2[0] / nbin)) / 100.0
        prof = (prof + sigma * torch.randn(prof.shape, generator=g, device=dev, dtype=torch.float64)).to(torch.float32)
        data = prof.reshape(nchan, nsub * nbin).contiguous()
        del prof
        ld = nsub * nbin
        out = torch.empty((nchan * nsub, 8), dtype=torch.float32, device=dev)
        spec1 = torch.from_numpy(one.spec).to(dev)
        specn = torch.from_numpy(per.spec).to(dev)

        def fit(spec, ntmpl):
            _lib.check(L.pss_toa_fit(data.data_ptr(), nchan, nsub, nbin, ld, spec.data_ptr(), ntmpl, K, out.data_ptr(), 8,
                                     st), "toa_fit")

        e = {"channels": nchan, "subints": nsub, "bins": nbin, "harmonics": K, "profiles": nchan * nsub,
             "path": "fft" if nbin in (32, 64, 128, 256, 512, 1024, 2048, 4096) else "direct",
             "data_bytes": nchan * ld * 4}
        e["toa_fit"] = timed(lambda: fit(spec1, 1))
        e["toa_fit"]["read_GBps"] = round(e["data_bytes"] / (e["toa_fit"]["ms"] * 1e-3) / 1e9, 1)
        e["toa_fit"]["us_per_profile"] = round(e["toa_fit"]["ms"] * 1e3 / (nchan * nsub), 4)
        fit(spec1, 1)
        torch.cuda.synchronize()
        o = out.cpu().numpy().astype(np.float64)
        d = o[:, 0] - tau.reshape(-1).cpu().numpy()
        d -= np.floor(d + 0.5)
        e["status_counts"] = [int((o[:, 7] == s).sum()) for s in (0, 1, 2)]
        e["median_snr"] = round(float(np.median(o[:, 6])), 1)
        e["pull_std"] = round(float((d / o[:, 1]).std()), 3)
        e["toa_fit_per_channel"] = timed(lambda: fit(specn, nchan))
        other = torch.empty_like(data)
        e["copy"] = timed(lambda: other.copy_(data))
        e["copy"]["moved_GBps"] = round(2 * e["data_bytes"] / (e["copy"]["ms"] * 1e-3) / 1e9, 1)
        del other
        Sc = torch.zeros(nbin // 2 + 1, dtype=torch.complex64, device=dev)
        Sc[1:K + 1] = torch.view_as_complex(spec1[0, 1:].contiguous()).conj()
        jmax = torch.empty(nchan * nsub, dtype=torch.int64, device=dev)

        def coarse():
            X = torch.fft.rfft(data.view(nchan * nsub, nbin), dim=1) * Sc
            jmax.copy_(torch.argmax(torch.fft.irfft(X, n=nbin, dim=1), dim=1))

        e["torch_coarse"] = timed(coarse)
        j = jmax.cpu().numpy()
        dj = o[:, 0] * nbin - j
        dj -= nbin * np.floor(dj / nbin + 0.5)
        e["coarse_agrees"] = bool((np.abs(dj) <= 1.0 + 1e-3).all())
        assert e["coarse_agrees"], "the kernel's tau and the torch composition's grid maximum differ"
        e["fit_over_copy"] = round(e["toa_fit"]["ms"] / e["copy"]["ms"], 2)
        e["torch_coarse_over_fit"] = round(e["torch_coarse"]["ms"] / e["toa_fit"]["ms"], 2)
        res["rows"].append(e)
        del data, out, jmax
        torch.cuda.empty_cache()
    bench_util.emit(res, args.out)


if __name__ == "__main__":
    main()
