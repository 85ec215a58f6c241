#!/usr/bin/env python
"""Time the fast folding search (pss_ffa_transform, pss_ffa_profile_search,
pss_ffa_scrunch) next to its yardsticks, measured in the same process, and
print one JSON line (optionally also to --out; profiles/ffa_search/ffa_bench.json
is such a run).

    python tools/ffa_bench.py [--bins 256] [--reps 7] [--out FILE]

One octave (lf = 0, base periods bins .. 2 bins - 1) of series of normal random
data (float32 [nser][T], row stride T rounded up to 4 samples) at the two
lengths of tools/accel_bench.py,
  * search : (2^20 - 1969) samples, 1 series;
  * chan   : (65536 - 24615) samples, 16 series.
Per shape:
  * transform          : pss_ffa_transform of the product library: the bottom
    of every tree in LDS, one launch for each level above it;
  * transform_unfused  : the same sources built with -DPSS_FFA_NO_FUSE=1, in
    which every level is one launch -- the A/B behind the LDS subtrees (the
    variant library is built on first use; both are loaded in this process and
    must give the same bits, unfused_equals_fused);
  * fused_threads      : the same sources built with
    -DPSS_FFA_FUSED_THREADS=256 and 1024 next to the product's 512 threads a
    workgroup of the LDS pass -- the A/B behind that size; same bits;
  * profile_search     : pss_ffa_profile_search of the transform's output, six
    widths, cells of 16 profiles;
  * scrunch            : pss_ffa_scrunch of the series with the mean
    subtracted, lf = 0 (what this octave runs) and lf = 4;
  * torch_composition  : what a user would otherwise write, for the first
    --comp-periods base periods: per level the indexed rows of the level below
    (index_select with host tables), the second rotated per row -- torch.roll
    takes one shift for the whole tensor, so the per-row roll is the gather a
    loop of rolls amounts to -- and an add.  Its output must equal the
    kernel's bit for bit (equals_composition; the tool asserts it), and it is
    compared with the kernel run on the same periods (transform_subset);
  * device_copy        : a plain device copy of the bytes of one level (all
    periods); the transform is reported as a multiple of levels x that;
  * harmonic           : Backend.harmonic_snr (16 harmonics) of the same rows,
    for context.
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

VARIANT, VARIANT_FLAGS = "ffa_nofuse", ["-DPSS_FFA_NO_FUSE=1"]
THREADS = (("256", "ffa_t256", ["-DPSS_FFA_FUSED_THREADS=256"]), ("1024", "ffa_t1024", ["-DPSS_FFA_FUSED_THREADS=1024"]))


def level_tables(np, m, p, d):
    """(H, T, b int64 [m], combine bool [m]) of depth d of the tree of m rows:
    the rows of depth d + 1 a row adds (H, and T rotated by b), or copies."""
    r = np.arange(m, dtype=np.int64)
    a = np.zeros(m, dtype=np.int64)
    mm = np.full(m, m, dtype=np.int64)
    for _ in range(d):
        h = mm // 2
        left = r < a + h
        split = mm > 1
        a = np.where(split & ~left, a + h, a)
        mm = np.where(split, np.where(left, h, mm - h), mm)
    comb = mm > 1
    h = mm // 2
    t = mm - h
    s = r - a
    den = np.maximum(2 * (mm - 1), 1)
    H = np.where(comb, a + (2 * s * (h - 1) + (mm - 1)) // den, r)
    T = np.where(comb, a + h + (2 * s * (t - 1) + (mm - 1)) // den, r)
    b = np.where(comb, ((2 * s * h + (mm - 1)) // den) % p, 0)
    return H, T, b, comb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cell", type=int, default=16)
    ap.add_argument("--nwidths", type=int, default=6)
    ap.add_argument("--comp-periods", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    from psrsigsim_amd import _lib, build
    from psrsigsim_amd.telescope import Backend, DedispersedPlane
    L = _lib.lib()
    Lu = _lib.load(build.build(variant=VARIANT, variant_flags=VARIANT_FLAGS, verbose=False))
    Lt = {t: _lib.load(build.build(variant=v, variant_flags=fl, verbose=False)) for t, v, fl in THREADS}
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.current_stream().cuda_stream
    B, cell, nw, ncomp = args.bins, args.cell, args.nwidths, args.comp_periods
    timed = functools.partial(bench_util.timed, reps=args.reps)

    res = {"reps": args.reps, "device": torch.cuda.get_device_name(dev), "library": os.path.basename(_lib.LIB_PATH),
           "unfused_library": "libpss_hip_%s.so (%s)" % (VARIANT, " ".join(VARIANT_FLAGS)), "bins": B, "rows": []}
    for name, T, nser in (("search", (1 << 20) - 1969, 1), ("chan", 65536 - 24615, 16)):
        ld = (T + 3) // 4 * 4
        x = torch.randn((nser, ld), dtype=torch.float32, device=dev)
        mean, var = Backend._trial_stats(x[:, :T], ld, 1024)
        mean32 = mean.to(torch.float32)
        rstd32 = (1.0 / torch.sqrt(var)).to(torch.float32)
        n, p0, npd = T, B, B
        ms = [n // (p0 + pi) for pi in range(npd)]
        levels = max(1, (ms[0] - 1).bit_length())
        words = nser * npd * n
        e = {"shape": name, "series": nser, "samples": T, "p0": p0, "np": npd, "m": [ms[-1], ms[0]], "levels": levels,
             "level_bytes": words * 4}
        y = torch.empty((nser, ld), dtype=torch.float32, device=dev)

        def scrunch(lf):
            _lib.check(L.pss_ffa_scrunch(x.data_ptr(), nser, T, ld, mean32.data_ptr(), lf, y.data_ptr(), ld, st),
                       "ffa_scrunch")

        e["scrunch_lf4"] = timed(lambda: scrunch(4))
        e["scrunch"] = timed(lambda: scrunch(0))
        out = torch.empty(words, dtype=torch.float32, device=dev)
        work = torch.empty(words, dtype=torch.float32, device=dev)

        def transform(lib, np_=npd):
            _lib.check(lib.pss_ffa_transform(y.data_ptr(), nser, n, ld, p0, np_, out.data_ptr(), work.data_ptr(), st),
                       "ffa_transform")

        out.zero_()                                        # (words [m p, n) of a block are written by neither route)
        e["transform_unfused"] = timed(lambda: transform(Lu))
        unfused = out.clone()
        out.zero_()
        e["transform"] = timed(lambda: transform(L))
        e["unfused_equals_fused"] = bool(torch.equal(unfused.view(torch.int32), out.view(torch.int32)))
        assert e["unfused_equals_fused"], "the fused and the unfused transform differ"
        del unfused
        # the workgroup of the LDS pass: 256 / 512 (the product) / 1024 threads
        want = out.clone()
        e["fused_threads"] = {"512": dict(e["transform"])}
        for t, lib in Lt.items():
            out.zero_()
            e["fused_threads"][t] = timed(lambda: transform(lib))
            e["fused_threads"][t]["same_bits"] = bool(torch.equal(want.view(torch.int32), out.view(torch.int32)))
            assert e["fused_threads"][t]["same_bits"]
        del want
        e["fused_over_unfused"] = round(e["transform"]["ms"] / e["transform_unfused"]["ms"], 3)
        e["device_copy"] = timed(lambda: work.copy_(out))
        e["device_copy"]["GBps"] = round(2 * words * 4 / (e["device_copy"]["ms"] * 1e-3) / 1e9, 1)
        e["transform_over_levels_x_copy"] = round(e["transform"]["ms"] / (levels * e["device_copy"]["ms"]), 3)
        e["unfused_over_levels_x_copy"] = round(e["transform_unfused"]["ms"] / (levels * e["device_copy"]["ms"]), 3)
        transform(L)
        # the profile search of the transform's output
        rm = torch.from_numpy(np.array([1.0 / np.sqrt(m) for m in ms]).astype(np.float32)).to(dev)
        nq = (ms[0] + cell - 1) // cell
        snr = torch.empty((nser * npd, nq), dtype=torch.float32, device=dev)
        code = torch.empty((nser * npd, nq), dtype=torch.int32, device=dev)
        phase = torch.empty_like(code)
        e["profile_search"] = timed(lambda: _lib.check(L.pss_ffa_profile_search(
            out.data_ptr(), nser, n, p0, npd, rstd32.data_ptr(), rm.data_ptr(), nw, cell, snr.data_ptr(),
            code.data_ptr(), phase.data_ptr(), nq, st), "ffa_profile_search"))
        e["profile_search"]["read_GBps"] = round(words * 4 / (e["profile_search"]["ms"] * 1e-3) / 1e9, 1)
        e["best_z"] = round(float(snr.max()), 3)
        del snr, code, phase
        # the composition, on the first ncomp periods, against the kernel on the same periods
        e["comp_periods"] = ncomp
        e["transform_subset"] = timed(lambda: transform(L, ncomp))
        want = out[:nser * ncomp * n].view(nser, ncomp, n).clone()
        tabs = []
        for pi in range(ncomp):
            p, m = p0 + pi, ms[pi]
            lev = []
            for d in range(max(1, (m - 1).bit_length()) - 1, -1, -1):
                H, Tt, b, comb = level_tables(np, m, p, d)
                rows = np.flatnonzero(comb)
                rot = (np.arange(p, dtype=np.int64)[None, :] + b[rows, None]) % p
                lev.append(tuple(torch.from_numpy(v).to(dev) for v in (rows, H[rows], Tt[rows], rot,
                                                                       np.flatnonzero(~comb))))
            tabs.append(lev)
        e["index_table_bytes"] = int(sum(v.numel() * 8 for lev in tabs for t in lev for v in t))
        comp_out = [None] * ncomp

        def comp():
            for pi in range(ncomp):
                p, m = p0 + pi, ms[pi]
                X = y[:, :m * p].reshape(nser, m, p)
                for rows, H, Tt, rot, cp in tabs[pi]:
                    nxt = torch.empty_like(X)
                    nxt[:, rows] = X.index_select(1, H) + torch.gather(X.index_select(1, Tt), 2,
                                                                       rot[None].expand(nser, -1, -1))
                    if cp.numel():
                        nxt[:, cp] = X.index_select(1, cp)
                    X = nxt
                comp_out[pi] = X

        e["torch_composition"] = timed(comp)
        e["equals_composition"] = all(
            bool(torch.equal(comp_out[pi].reshape(nser, -1).view(torch.int32),
                             want[:, pi, :ms[pi] * (p0 + pi)].view(torch.int32))) for pi in range(ncomp))
        assert e["equals_composition"], "the kernel and the torch composition differ"
        e["torch_over_kernel"] = round(e["torch_composition"]["ms"] / e["transform_subset"]["ms"], 2)
        e["kernel_beats_torch"] = bool(e["transform_subset"]["ms"] < e["torch_composition"]["ms"])
        assert e["kernel_beats_torch"], "the torch composition is faster than the kernel"
        del tabs, comp_out, want, out, work
        torch.cuda.empty_cache()
        # for context: the 16-harmonic search of the same rows
        plane = DedispersedPlane(x[:, :T], np.arange(float(nser)), np.zeros((nser, 1), dtype=np.int32), 0.01, 1400.0, 0)
        be = Backend(samprate=0.01, name="bench")
        mean_h, std_h = mean.cpu().numpy(), torch.sqrt(var).cpu().numpy()
        e["harmonic"] = timed(lambda: be.harmonic_snr(plane, nharm=16, mean=mean_h, std=std_h))
        e["transform_plus_search_over_harmonic"] = round((e["transform"]["ms"] + e["profile_search"]["ms"])
                                                         / e["harmonic"]["ms"], 1)
        res["rows"].append(e)
        del x, y, plane
        torch.cuda.empty_cache()
    bench_util.emit(res, args.out)


if __name__ == "__main__":
    main()
