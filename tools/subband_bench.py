#!/usr/bin/env python
"""Time the two-stage sub-band dedispersion (pss_dedisperse_banded, as
Backend.subband_dedisperse launches it) next to the direct sum and to the same
two stages composed from launches of the existing kernel, in one process, and
print one JSON line (optionally also to --out).

    python tools/subband_bench.py [--nchan 2048] [--log2n 20] [--ndm 1024] [--reps 7] [--out FILE]

Shapes (float32 [chan][time], 1200-1600 MHz, trial DMs 0 .. 100 pc/cm^3):
  * search      : nchan x 2^log2n samples at 64 us, the plan subband_plan picks at max_smear = 2;
  * search_64x16: the same data with nsub = 64, group = 16;
  * chan        : the channeliser's product of 2^28 voltages at C = 2048 (2048 x 65536 samples at 195.3 kHz), the
    plan subband_plan picks.
Per shape, medians of --reps calls after a warm-up call, the entries measured in
turn (bench_util.timed_alternating; device events):
  * stage1, stage2 : every chunk's launch of that stage (chunks of whole groups within max_bytes = 2^31, as the API),
    and their sum;
  * two_stage      : the chunks' launches in the API's order (stage 1, stage 2, next chunk);
  * direct         : pss_dedisperse on the same trials (the exact table);
  * composed       : the same two stages from launches of pss_dedisperse -- one per band and chunk, then one per
    group -- and its stages;
  * device_copy    : a plain device copy of the input bytes.
additions and bytes are computed from the shapes (bytes: what the workgroups request, the 8 trials of a workgroup
sharing a row; the input's re-reads by the bands' and groups' workgroups of one time tile are meant to hit in L2).
max_rel_diff_vs_direct_over_e compares the plane with pss_dedisperse on the effective table (same sum, other order of
the float32 additions).  Needs the GPU: there is no CPU path.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_util  # noqa: E402  (tools/, next to this file)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nchan", type=int, default=2048)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--ndm", type=int, default=1024)
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

    res = {"reps": args.reps, "device": torch.cuda.get_device_name(dev), "max_bytes": 2 ** 31, "shapes": []}
    dms = np.linspace(0.0, 100.0, args.ndm)
    shapes = [("search", args.nchan, 1 << args.log2n, 1.0 / 64.0, None, None),
              ("search_64x16", args.nchan, 1 << args.log2n, 1.0 / 64.0, 64, 16),
              ("chan", 2048, (1 << 28) // 4096, 800.0 / 4096.0, None, None)]
    for name, C, N, rate, nsub, group in shapes:
        sig = FilterBankSignal(1400, 400, Nsubband=C, sample_rate=1000.0, fold=False)
        sig._samprate = make_quant(rate, 'MHz')                # (set here: the constructor warns below Nyquist)
        sig._buf, sig._ncols = object(), N                     # (the plan reads the length only)
        D = Backend.dedisperse_delays(sig, dms)
        p = Backend.subband_plan(sig, dms, nsub=nsub, group=group, max_smear=2.0)
        chunks = Backend._subband_chunks(p, 2 ** 31)
        ndm, ns, grp, band = D.shape[0], p.nsub, p.group, C // p.nsub
        md, T1, T = int(D.max()), p.T1, p.T
        Td = N - md
        ld1, ldo, ldd = (T1 + 3) // 4 * 4, (T + 3) // 4 * 4, (Td + 3) // 4 * 4
        gmax = max(hi - lo for lo, hi in chunks)

        x = torch.rand((C, N), dtype=torch.float32, device=dev)
        t1 = torch.from_numpy(p.d1).to(dev)
        t2 = torch.from_numpy(p.d2).to(dev)
        # the composition's stage 1 takes a band's columns of d1 as a table of its own
        t1b = torch.from_numpy(np.ascontiguousarray(p.d1.reshape(-1, ns, band).transpose(1, 0, 2))).to(dev)
        tD = torch.from_numpy(D).to(dev)
        tE = torch.from_numpy(p.delays).to(dev)
        sub = torch.empty((gmax, ns, ld1), dtype=torch.float32, device=dev)
        out = torch.empty((ndm, ldo), dtype=torch.float32, device=dev)
        out_c = torch.empty((ndm, ldo), dtype=torch.float32, device=dev)
        out_d = torch.empty((ndm, max(ldd, ldo)), dtype=torch.float32, device=dev)

        def stage1(lo, hi):
            _lib.check(L.pss_dedisperse_banded(x.data_ptr(), 1, C * N, C, N, N, t1[lo:hi].data_ptr(), hi - lo, hi - lo,
                                               p.m1, band, sub.data_ptr(), ld1, st), "dedisperse_banded")

        def stage2(lo, hi, dst=out):
            j0, j1 = lo * grp, min(ndm, hi * grp)
            _lib.check(L.pss_dedisperse_banded(sub.data_ptr(), hi - lo, ns * ld1, ns, T1, ld1, t2[j0:j1].data_ptr(),
                                               j1 - j0, grp, p.m2, ns, dst[j0:j1].data_ptr(), ldo, st),
                       "dedisperse_banded")

        def comp1(lo, hi):
            for s in range(ns):
                _lib.check(L.pss_dedisperse(x[s * band:].data_ptr(), band, N, N, t1b[s, lo:hi].data_ptr(), hi - lo,
                                            p.m1, sub[:, s].data_ptr(), ns * ld1, st), "dedisperse")

        def comp2(lo, hi):
            for g in range(lo, hi):
                j0, j1 = g * grp, min(ndm, (g + 1) * grp)
                _lib.check(L.pss_dedisperse(sub[g - lo].data_ptr(), ns, T1, ld1, t2[j0:j1].data_ptr(), j1 - j0, p.m2,
                                            out_c[j0:j1].data_ptr(), ldo, st), "dedisperse")

        def every(*stages):
            def run():
                for lo, hi in chunks:
                    for f in stages:
                        f(lo, hi)
            return run

        def direct(tab=tD, mdel=md, ld=ldd):
            _lib.check(L.pss_dedisperse(x.data_ptr(), C, N, N, tab.data_ptr(), ndm, mdel, out_d.data_ptr(), ld, st),
                       "dedisperse")

        dst = torch.empty_like(x)
        t = bench_util.timed_alternating({
            "stage1": every(stage1), "stage2": every(stage2), "two_stage": every(stage1, stage2), "direct": direct,
            "composed_stage1": every(comp1), "composed_stage2": every(comp2), "composed": every(comp1, comp2),
            "device_copy": lambda: dst.copy_(x)}, args.reps)
        del dst
        torch.cuda.empty_cache()

        ngroups = int(p.d1.shape[0])
        wg1 = sum(-(-(hi - lo) // 8) for lo, hi in chunks)         # stage 1: workgroups' trial groups over the chunks
        wg2 = sum(-(-(min(ndm, (g + 1) * grp) - g * grp) // 8) for g in range(ngroups))
        e = {"shape": name, "nchan": C, "nsamp": N, "ndm": ndm, "samprate_MHz": rate, "nsub": ns, "group": grp,
             "ngroups": ngroups, "chunks": len(chunks), "smear": p.smear, "m1": p.m1, "m2": p.m2,
             "max_delay_direct": md, "out_samples": T, "out_samples_direct": Td,
             "additions_direct": C * Td * ndm, "additions_stage1": ngroups * C * T1, "additions_stage2": ndm * ns * T,
             "adds_ratio": round(p.adds_subband / p.adds_direct, 4),
             "bytes_input_requested_stage1": wg1 * C * N * 4, "bytes_workspace_written": ngroups * ns * T1 * 4,
             "bytes_workspace_requested_stage2": wg2 * ns * T1 * 4, "bytes_plane_written": ndm * T * 4,
             "bytes_input_requested_direct": -(-ndm // 8) * C * N * 4, "workspace_bytes": gmax * ns * ld1 * 4}
        e.update(t)
        e["stages_sum_ms"] = round(t["stage1"]["ms"] + t["stage2"]["ms"], 4)
        e["device_copy"]["GBps"] = round(2 * C * N * 4 / (t["device_copy"]["ms"] * 1e-3) / 1e9, 1)
        e["direct_over_two_stage"] = round(t["direct"]["ms"] / t["two_stage"]["ms"], 2)
        e["composed_over_two_stage"] = round(t["composed"]["ms"] / t["two_stage"]["ms"], 2)
        e["two_stage_beats_direct"] = bool(t["two_stage"]["ms"] < t["direct"]["ms"])
        e["two_stage_beats_composed"] = bool(t["two_stage"]["ms"] < t["composed"]["ms"])
        # the plane against the direct sum over the effective table, and the composition's bits
        every(stage1, stage2)()
        every(comp1, comp2)()
        direct(tE, p.m1 + p.m2, ldo)
        torch.cuda.synchronize()
        ref = out_d.view(-1)[:ndm * ldo].view(ndm, ldo)[:, :T]
        e["max_rel_diff_vs_direct_over_e"] = float(((out[:, :T] - ref).abs().max() / ref.abs().max()).item())
        e["composed_same_bits"] = bool(torch.equal(out[:, :T], out_c[:, :T]))
        res["shapes"].append(e)
        del x, sub, out, out_c, out_d, ref
        torch.cuda.empty_cache()
    bench_util.emit(res, args.out)


if __name__ == "__main__":
    main()
