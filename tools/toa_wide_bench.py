#!/usr/bin/env python
"""Time the wideband fit (pss_toa_wide_fit) and its stages next to their
yardsticks, measured in the same process, and print one JSON line (optionally
also to --out; profiles/toa_wide/toa_wide_bench.json is such a run).

    python tools/toa_wide_bench.py [--nchan 2048] [--nsub 15] [--reps 7] [--out FILE]

Profiles: toa_bench.py's three-component template, delayed in every channel by
phi0_n + phi_s + kappa_n d_s (a 1200 .. 1600 MHz band, one phase and one DM
offset of up to a third of a bin across the band per sub-integration) under
Gaussian noise at b / b_err = 3 per channel -- the regime the wideband fit is
for -- float32 [nchan][nsub * nbin], at 2048 bins (the FFT path of the spectrum
stage) and at 2000 bins (the direct path).  Per shape:
  * wide_fit : the whole fit, ndm = 1;
  * stage_spectrum, stage_start (channel lists, coarse trial, start),
    stage_rounds (32 x evaluation + step; finished sub-integrations return at
    once), stage_finish : pss_toa_wide_stages on the workspace of a whole fit;
  * toa_fit : pss_toa_fit on the same data;
  * copy_data, copy_x : plain device copies of the profile bytes and of the
    bytes of the X workspace, which one evaluation streams once.
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
    ap.add_argument("--snr", type=float, default=3.0)
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
           "snr_per_channel": args.snr, "rows": []}
    for nbin in args.nbins:
        ph = np.arange(nbin) / nbin
        tm = sum(a * np.exp((np.cos(2 * np.pi * (ph - c)) - 1) / (2 * np.pi * w) ** 2)
                 for c, w, a in ((0.30, 0.03, 1.0), (0.36, 0.05, 0.45), (0.22, 0.08, 0.2)))
        one = Backend.toa_template(tm, nbin)
        K = one.K
        rng = np.random.default_rng(7)
        f = np.linspace(1200.0, 1600.0, nchan)
        kappa = 40.0 * (f[0] / f) ** 2
        span = float(kappa.max() - kappa.min())
        phi0 = rng.uniform(-0.5, 0.5, nchan)
        phi = rng.uniform(-0.5, 0.5, nsub)
        d = rng.uniform(-1.0, 1.0, nsub) / (3.0 * nbin * span)
        tau = torch.from_numpy(phi0[:, None] + phi[None, :] + kappa[:, None] * d[None, :]).to(dev)[:, :, None]
        g = torch.Generator(device=dev)
        g.manual_seed(7)
        S = torch.from_numpy(np.fft.rfft(tm)).to(dev)
        k = torch.arange(S.shape[0], device=dev, dtype=torch.float64)
        prof = torch.fft.irfft(S * torch.exp(-2j * np.pi * k * tau), n=nbin)
        sigma = float(np.sqrt(2 * one.S2[0] / nbin)) / args.snr
        prof = (prof + sigma * torch.randn(prof.shape, generator=g, device=dev, dtype=torch.float64)).to(torch.float32)
        data = prof.reshape(nchan, nsub * nbin).contiguous()
        del prof, tau
        ld = nsub * nbin
        spec = torch.from_numpy(one.spec).to(dev)
        kap = torch.from_numpy(kappa).to(dev)
        ph0 = torch.from_numpy(phi0 - np.floor(phi0 + 0.5)).to(dev)
        wt = torch.full((nchan, nsub), 2.0 / (nbin * sigma * sigma), dtype=torch.float32, device=dev)
        need = int(L.pss_toa_wide_workspace_bytes(nchan, nsub, nbin, K, 1))
        work = torch.empty((need,), dtype=torch.uint8, device=dev)
        out = torch.empty((nsub, 10), dtype=torch.float64, device=dev)
        rows = torch.empty((nchan, nsub, 4), dtype=torch.float32, device=dev)
        nb = torch.empty((nchan * nsub, 8), dtype=torch.float32, device=dev)

        def stages(first, last):
            _lib.check(L.pss_toa_wide_stages(data.data_ptr(), nchan, nsub, nbin, ld, spec.data_ptr(), 1, K,
                                             kap.data_ptr(), ph0.data_ptr(), wt.data_ptr(), 1, 0.0, out.data_ptr(), 10,
                                             rows.data_ptr(), 4, work.data_ptr(), need, first, last, st),
                       "toa_wide_stages")

        def narrow():
            _lib.check(L.pss_toa_fit(data.data_ptr(), nchan, nsub, nbin, ld, spec.data_ptr(), 1, K, nb.data_ptr(), 8,
                                     st), "toa_fit")

        x_bytes = nchan * nsub * K * 8
        e = {"channels": nchan, "subints": nsub, "bins": nbin, "harmonics": K,
             "path": "fft" if nbin in (32, 64, 128, 256, 512, 1024, 2048, 4096) else "direct",
             "data_bytes": nchan * ld * 4, "x_bytes": x_bytes, "workspace_bytes": need}
        e["wide_fit"] = timed(lambda: stages(0, 3))
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        dphi = o[:, 0] - phi
        dphi -= np.floor(dphi + 0.5)
        e["status_counts"] = [int((o[:, 9] == s).sum()) for s in (0, 1, 2)]
        e["evaluations_mean"] = round(float(o[:, 8].mean()), 2)
        e["evaluations_max"] = int(o[:, 8].max())
        e["phi_pull_max"] = round(float(np.abs(dphi / o[:, 1]).max()), 2)
        e["d_pull_max"] = round(float(np.abs((o[:, 2] - d) / o[:, 3]).max()), 2)
        e["chi2r_mean"] = round(float((o[:, 5] / o[:, 6]).mean()), 4)
        for name, (a, b) in (("stage_spectrum", (0, 0)), ("stage_start", (1, 1)), ("stage_rounds", (2, 2)),
                             ("stage_finish", (3, 3))):
            e[name] = timed(lambda: stages(a, b))
        # (stage_rounds above ran on finished sub-integrations: every launch returns at once; the rounds of a
        # fresh fit are the whole fit less the other three stages)
        e["rounds_of_a_fit_ms"] = round(e["wide_fit"]["ms"] - e["stage_spectrum"]["ms"] - e["stage_start"]["ms"]
                                        - e["stage_finish"]["ms"], 4)
        e["toa_fit"] = timed(narrow)
        other = torch.empty_like(data)
        e["copy_data"] = timed(lambda: other.copy_(data))
        del other
        xa = torch.empty((x_bytes,), dtype=torch.uint8, device=dev)
        xb = torch.empty_like(xa)
        e["copy_x"] = timed(lambda: xb.copy_(xa))
        del xa, xb
        e["fit_over_toa_fit"] = round(e["wide_fit"]["ms"] / e["toa_fit"]["ms"], 2)
        e["fit_over_copy_x"] = round(e["wide_fit"]["ms"] / e["copy_x"]["ms"], 2)
        e["evaluation_over_copy_x"] = round(e["stage_finish"]["ms"] / e["copy_x"]["ms"], 2)
        res["rows"].append(e)
        del data, out, rows, nb, work
        torch.cuda.empty_cache()
    bench_util.emit(res, args.out)


if __name__ == "__main__":
    main()
