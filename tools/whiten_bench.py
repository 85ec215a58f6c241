#!/usr/bin/env python
"""Time the spectrum whitening (pss_spectrum_medians, pss_spectrum_whiten)
next to its yardsticks, measured in the same process, and print one JSON line
(optionally also to --out; profiles/whiten/whiten_bench.json is such a run).

    python tools/whiten_bench.py [--ndm 64] [--reps 7] [--out FILE]

Spectra (complex64 [ndm][nbin + 1], the transform of unit white noise plus
0.05 cumsum(white), rows as torch.fft.rfft leaves them: every other row off
the 16-B grid) of 2^19 and 2^20 bins with the default plan of
Backend.whiten_plan.  Per shape:
  * medians, whiten, whiten_inplace : the two kernels of the product library,
    the whitening into a second tensor and in place, both without a mask;
  * whiten_inplace_zap : the whitening in place with a mask (Backend.zap_mask
    at 10 kHz: 60 Hz and its harmonics up to 3 kHz, 1 Hz wide each), which
    adds one byte load a bin;
  * copy_8B, copy_16B : a plain device copy that moves the same bytes -- the
    medians read 8 B a bin (a copy of 4 B a bin reads 4 and writes 4), the
    whitening reads 8 and writes 8 (a copy of the spectrum);
  * torch_medians, torch_whiten : what a user would otherwise write.  The
    powers are gathered into blocks padded to [nblk, 256] -- with -inf and +inf
    in such numbers that the lower median of every block stands at the same
    rank, since kthvalue takes one k for the whole tensor -- and kthvalue
    selects; the index of the bracketing centres comes from searchsorted (a
    table made once, outside the timing, like the plan) and lerp interpolates.
    The medians must equal the kernel's bit for bit; lerp rounds differently
    from the contract, so the whitened spectrum is compared to 1e-5;
  * rfft, harmonic : the transform and the 16-harmonic search of the same
    rows, the rest of Backend.harmonic_snr: whiten_share is the whitening's
    part of the four.
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

LN2 = 0.6931471805599453


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ndm", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cell", type=int, default=32)
    ap.add_argument("--log2", type=int, nargs="+", default=[19, 20])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from psrsigsim_amd import _lib
    from psrsigsim_amd.telescope import Backend
    L = _lib.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    ndm, cell = args.ndm, args.cell
    timed = functools.partial(bench_util.timed, reps=args.reps)
    gbps = lambda nbytes, t: round(nbytes / (t["ms"] * 1e-3) / 1e9, 1)      # noqa: E731

    res = {"reps": args.reps, "device": torch.cuda.get_device_name(dev), "library": os.path.basename(_lib.LIB_PATH),
           "rows": []}
    for lg in args.log2:
        nbin = 1 << lg
        nfft = 2 * nbin
        plan = Backend.whiten_plan(nbin)
        nblk = plan.nblk
        w = np.diff(plan.edges)
        x = torch.randn((ndm, nfft), dtype=torch.float32, device=dev)
        x += 0.05 * torch.cumsum(torch.randn((ndm, nfft), dtype=torch.float32, device=dev), dim=1)
        x -= x.mean(dim=1, keepdim=True)
        e = {"trials": ndm, "bins": nbin, "blocks": nblk, "blocks_of_wmax": int((w == plan.wmax).sum()),
             "spectrum_bytes": ndm * nbin * 8}
        e["rfft"] = timed(lambda: torch.fft.rfft(x, n=nfft))
        spec = torch.fft.rfft(x, n=nfft)
        del x
        ld = int(spec.shape[1])
        edges_d = torch.from_numpy(plan.edges).to(dev)
        med = torch.empty((ndm, nblk), dtype=torch.float32, device=dev)
        out = torch.empty_like(spec)
        work = spec.clone()

        def k_med():
            _lib.check(L.pss_spectrum_medians(spec.data_ptr(), ndm, nbin, ld, edges_d.data_ptr(), nblk, med.data_ptr(),
                                              nblk, st), "spectrum_medians")

        def k_wh(src, dst, zap=None):
            _lib.check(L.pss_spectrum_whiten(src.data_ptr(), ndm, nbin, ld, edges_d.data_ptr(), nblk, med.data_ptr(),
                                             nblk, None if zap is None else zap.data_ptr(), dst.data_ptr(), ld, st),
                       "spectrum_whiten")

        e["medians"] = timed(k_med)
        e["medians"]["read_GBps"] = gbps(e["spectrum_bytes"], e["medians"])
        e["whiten"] = timed(lambda: k_wh(spec, out))
        e["whiten"]["moved_GBps"] = gbps(2 * e["spectrum_bytes"], e["whiten"])
        e["whiten_inplace"] = timed(lambda: k_wh(work, work))
        mask = Backend.zap_mask(nfft, 0.01, [(60.0 * h - 0.5, 60.0 * h + 0.5) for h in range(1, 51)])
        zap_d = torch.from_numpy(mask).to(dev)
        e["zapped_bins"] = int(mask.sum())
        e["whiten_inplace_zap"] = timed(lambda: k_wh(work, work, zap_d))
        del work
        # a device copy of the same bytes
        half_a = torch.empty((ndm, nbin), dtype=torch.float32, device=dev)
        half_b = torch.empty_like(half_a)
        e["copy_8B"] = timed(lambda: half_b.copy_(half_a))
        e["copy_8B"]["moved_GBps"] = gbps(e["spectrum_bytes"], e["copy_8B"])
        del half_a, half_b
        full = torch.empty_like(spec)
        e["copy_16B"] = timed(lambda: full.copy_(spec))
        e["copy_16B"]["moved_GBps"] = gbps(2 * ndm * ld * 8, e["copy_16B"])
        del full
        torch.cuda.empty_cache()
        # the composition: padded blocks and kthvalue, searchsorted's table and lerp
        slot = np.arange(256, dtype=np.int64)[None, :]
        idx = np.minimum(plan.edges[:-1, None] + slot, nbin - 1)
        n_neg = 127 - (w - 1) // 2
        pad = np.where(slot < (w + n_neg)[:, None], -np.inf, np.inf).astype(np.float32)
        valid_d = torch.from_numpy(slot < w[:, None]).to(dev)
        idx_d = torch.from_numpy(idx).to(dev).view(-1)
        pad_d = torch.from_numpy(pad).to(dev)
        d = torch.from_numpy(plan.edges[:-1] + plan.edges[1:] - 1).to(dev)
        k2 = 2 * torch.arange(nbin, dtype=torch.int64, device=dev)
        b = (torch.searchsorted(d, k2, right=True) - 1).clamp(0, max(nblk - 2, 0))
        b1 = (b + 1).clamp(max=nblk - 1)
        f = ((k2 - d[b]).to(torch.float32) / (d[b1] - d[b]).clamp(min=1).to(torch.float32)).clamp(0.0, 1.0)
        del k2
        comp_med = torch.empty_like(med)
        comp_out = torch.empty_like(spec)

        def t_med():
            sv = torch.view_as_real(spec[:, :nbin])
            P = sv[..., 0] * sv[..., 0] + sv[..., 1] * sv[..., 1]
            blocks = torch.where(valid_d, P[:, idx_d].view(ndm, nblk, 256), pad_d)
            comp_med.copy_(torch.kthvalue(blocks, 128, dim=-1).values)

        def t_wh():
            norm = torch.lerp(comp_med[:, b], comp_med[:, b1], f)
            s = torch.where((norm > 0) & torch.isfinite(norm), torch.sqrt(LN2 / norm), torch.zeros_like(norm))
            s[:, :plan.kstart] = 0
            comp_out[:, :nbin] = spec[:, :nbin] * s

        e["torch_medians"] = timed(t_med)
        e["torch_whiten"] = timed(t_wh)
        e["padded_block_bytes"] = ndm * nblk * 256 * 4
        e["medians_equal_composition"] = bool(torch.equal(med.view(torch.int32), comp_med.view(torch.int32)))
        assert e["medians_equal_composition"], "the kernel's medians and the torch composition differ"
        a, c = torch.view_as_real(out[:, :nbin]), torch.view_as_real(comp_out[:, :nbin])
        err = float(((a - c).abs() / (c.abs() + 1e-30)).max())
        e["whiten_max_rel_diff_to_composition"] = err
        assert err < 1e-5, "the whitening kernel and the torch composition differ by %g" % err
        P = (a * a).sum(dim=-1)[:, 64:]
        e["whitened_mean_power"] = round(float(P.mean()), 4)
        del comp_out, a, c, P, idx_d, pad_d, valid_d, f, b, b1
        torch.cuda.empty_cache()
        e["torch_over_kernel"] = round((e["torch_medians"]["ms"] + e["torch_whiten"]["ms"])
                                       / (e["medians"]["ms"] + e["whiten_inplace"]["ms"]), 2)
        e["medians_over_copy"] = round(e["medians"]["ms"] / e["copy_8B"]["ms"], 2)
        e["whiten_over_copy"] = round(e["whiten_inplace"]["ms"] / e["copy_16B"]["ms"], 2)
        # the rest of harmonic_snr on the same rows
        nq = (nbin + cell - 1) // cell
        q_ld = (nq + 15) // 16 * 16
        scale32 = torch.ones(ndm, dtype=torch.float32, device=dev)
        snr = torch.empty((ndm, q_ld), dtype=torch.float32, device=dev)
        code = torch.empty((ndm, q_ld), dtype=torch.int32, device=dev)
        hwork = torch.empty(ndm * nbin, dtype=torch.float32, device=dev)
        e["harmonic"] = timed(lambda: _lib.check(L.pss_harmonic_search(
            out.data_ptr(), ndm, nbin, ld, scale32.data_ptr(), 5, 1, cell, snr.data_ptr(), code.data_ptr(), q_ld,
            hwork.data_ptr(), st), "harmonic_search"))
        own = e["medians"]["ms"] + e["whiten_inplace"]["ms"]
        e["whiten_share"] = round(own / (own + e["rfft"]["ms"] + e["harmonic"]["ms"]), 3)
        res["rows"].append(e)
        del spec, out, med, comp_med, snr, code, hwork
        torch.cuda.empty_cache()
    bench_util.emit(res, args.out)


if __name__ == "__main__":
    main()
