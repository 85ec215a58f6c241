// pss_accel.hip -- time-domain resampling of dedispersed series for trial
// accelerations (extension, no reference counterpart): output row r is series
// i(r) read at the quadratically stretched times
//
//   idx_r(t) = t + sg(r) s_r(t),  s_r(t) = (t (T - t) K(r) + 2^63) >> 64,
//
// integers only (include/pss_hip.h has the definition and the proof of its
// bounds).  A pure data-movement kernel.
//
//   k_accel_resample<OVEC> : a workgroup of 256 threads owns kAcTB = 2048
//       output times of kAcNR = 8 consecutive rows.  Lanes run along time in
//       runs of 4: thread i holds times t0 + 4 (i + 256 k) .. + 3, k < 2, of
//       each row, so that a run leaves as one 16-B store (OVEC: `out` and
//       out_ld on the 16-B grid; dword stores otherwise -- the same bits).
//       Shift: a thread evaluates the 128-bit product at the two ends of a
//       run.  s is monotone on a run that does not hold the apex T / 2 of
//       t (T - t), so equal ends make the run a shifted copy; any other run is
//       evaluated per sample.
//       Source: idx_r is non-decreasing in t, so row r reads the source range
//       [idx_r(t0), idx_r(t0 + len - 1)] (wave-uniform, scalar arithmetic).
//       With i0 the series of the group's first row and wlo the lowest source
//       index of the rows that read i0,
//         staged  (i(r) = i0 and the range ends inside the window of kAcWin =
//                 4096 floats that begins at wlo, moved down to the 16-B grid
//                 of the address): the window is copied to LDS once for all
//                 such rows (stage_window, pss_window.hpp: 16-B loads where
//                 the window's whole 16-B groups lie inside [0, T) of the
//                 row, element loads where a group straddles the row's
//                 ends) and the outputs are gathered from LDS;
//         direct  (another series, or a range past the window): the outputs
//                 are gathered from global memory.
//       The values are the same by either route: every output is one word of
//       x, moved as bits (sub == NULL) or through one __fsub_rn.  No atomics,
//       no workspace; nothing depends on alignment, pitch or the row's
//       position.
//       Logical workgroup index = time tile * (row groups) + row group, dealt
//       to the XCDs in contiguous runs (the groups of one series -- more than
//       8 accelerations -- run side by side on one XCD and share its L2).
//   -DPSS_ACCEL_NO_STAGE=1 builds the A/B variant in which every row goes the
//       direct route, -DPSS_ACCEL_RUNS=1 / 4 the variants with tiles of 1024 /
//       4096 times and windows of twice that (tools/accel_bench.py; DESIGN.md
//       section 9).  The product is built with neither.
#include "pss_common.hpp"
#include "pss_window.hpp"

using namespace pss;

static constexpr int kAcThreads = 256;
static constexpr int kAcRun = 4;                          // consecutive outputs of a thread (one 16-B store)
#ifndef PSS_ACCEL_RUNS
#define PSS_ACCEL_RUNS 2
#endif
static constexpr int kAcRuns = PSS_ACCEL_RUNS;            // runs per thread and row
static constexpr int kAcTB = kAcThreads * kAcRun * kAcRuns;   // output times per workgroup (2048)
static constexpr int kAcNR = 8;                           // rows per workgroup
static constexpr int kAcWin = 2 * kAcTB;                  // staged window, floats (4096)
// a row's own range always fits: idx steps by at most 2, but over a tile by at
// most len + (s(t0 + len - 1) - s(t0)) <= len + len / 2 + 1, plus 3 to the grid
static_assert(kAcTB + kAcTB / 2 + 1 + 3 <= kAcWin, "a single row fits the window");

struct AcArgs {
    int64_t ld, out_ld;
    uint64_t kmax;                                        // floor(2^63 / T)
    int32_t T, n_out, nser, nrows, ngroups;
};

// s(t) = (t (T - t) K + 2^63) >> 64: the high word of the product plus the
// carry of the rounding, which is the low word's top bit.  K <= 2^63 / T, so
// s <= T / 8 + 1 fits 32 bits.
__device__ __forceinline__ uint32_t ac_shift(uint32_t t, uint32_t T, uint64_t K) {
    const uint64_t u = (uint64_t)t * (uint64_t)(T - t);
    return (uint32_t)(__umul64hi(u, K) + ((u * K) >> 63));
}

__device__ __forceinline__ int32_t ac_clamp(int64_t v, int32_t T) {
    return (int32_t)min(max(v, (int64_t)0), (int64_t)T - 1);
}

__device__ __forceinline__ int32_t ac_index(int32_t t, int32_t T, uint64_t K, int sg) {
    return ac_clamp((int64_t)t + sg * (int64_t)ac_shift((uint32_t)t, (uint32_t)T, K), T);
}

// K(r), sg(r) of a table entry
__device__ __forceinline__ uint64_t ac_step(int64_t kappa, uint64_t kmax, int &sg) {
    sg = kappa < 0 ? -1 : 1;
    const uint64_t mag = kappa < 0 ? (uint64_t)0 - (uint64_t)kappa : (uint64_t)kappa;
    return min(mag, kmax);
}

template <bool OVEC>
__global__ __launch_bounds__(kAcThreads) void k_accel_resample(const uint32_t *__restrict__ x,
                                                               const int32_t *__restrict__ src,
                                                               const int64_t *__restrict__ kappa,
                                                               const float *__restrict__ sub,
                                                               uint32_t *__restrict__ out, AcArgs a) {
    __shared__ __align__(16) uint32_t win[kAcWin];
    const int tid = threadIdx.x;
    const uint2 id = xcd_run_pair((unsigned)a.ngroups);
    const int g = (int)id.y;
    const int32_t t0 = (int32_t)id.x * kAcTB;
    const int r0 = g * kAcNR;
    const int nr = min(kAcNR, a.nrows - r0);                   // rows of this group (>= 1)
    const int len = min(kAcTB, a.n_out - t0);                  // times of this tile (>= 1)
    const int32_t T = a.T;
    PSS_DASSERT(nr >= 1 && len >= 1 && t0 >= 0 && t0 + len <= a.n_out && a.n_out <= T);

    // the source ranges of the group's rows (wave-uniform)
    int32_t si[kAcNR], lo[kAcNR], hi[kAcNR];
#pragma unroll
    for (int j = 0; j < kAcNR; ++j) {
        // (a ragged group repeats its last row)
        const int jj = r0 + min(j, nr - 1);
        int sg;
        const uint64_t K = ac_step(kappa[jj], a.kmax, sg);
        si[j] = min(max(src[jj], 0), a.nser - 1);
        lo[j] = ac_index(t0, T, K, sg);
        hi[j] = ac_index(t0 + len - 1, T, K, sg);
        PSS_DASSERT(lo[j] <= hi[j]);
    }
    int32_t wlo = lo[0];
#pragma unroll
    for (int j = 1; j < kAcNR; ++j)
        if (si[j] == si[0]) wlo = min(wlo, lo[j]);
    const uint32_t *row0 = x + (int64_t)si[0] * a.ld;
    // slot 0 of the window holds source index wb: wlo moved down to the 16-B
    // grid of the address
    const int64_t wb = (int64_t)wlo - (int64_t)(((uintptr_t)(row0 + wlo) >> 2) & 3);
    unsigned staged = 0;
    int need = 0;
#pragma unroll
    for (int j = 0; j < kAcNR; ++j) {
#ifndef PSS_ACCEL_NO_STAGE
        if (si[j] == si[0] && (int64_t)hi[j] - wb < kAcWin) {
            staged |= 1u << j;
            need = max(need, (int)((int64_t)hi[j] - wb) + 1);
        }
#endif
    }
    if (need > 0) {
        // (row0 + wb is on the 16-B grid by construction, VEC; wb may be as low as -3, HEAD)
        stage_window<kAcThreads, kAcWin, true, true>(win, row0, wb, need, T, tid);
        __syncthreads();
    }

    for (int j = 0; j < nr; ++j) {
        int sg;
        const uint64_t K = ac_step(kappa[r0 + j], a.kmax, sg);
        const int32_t i = min(max(src[r0 + j], 0), a.nser - 1);
        const uint32_t *row = x + (int64_t)i * a.ld;
        const bool st = (staged >> j) & 1u;
        const float sb = sub ? sub[r0 + j] : 0.0f;
        uint32_t *o = out + (int64_t)(r0 + j) * a.out_ld + t0;
#pragma unroll
        for (int k = 0; k < kAcRuns; ++k) {
            const int tl = kAcRun * (tid + k * kAcThreads);
            if (tl >= len) continue;
            const int nv = min(kAcRun, len - tl);              // outputs of this run
            const int32_t t = t0 + tl, tb = t + nv - 1;
            const uint32_t sa = ac_shift((uint32_t)t, (uint32_t)T, K);
            const uint32_t se = ac_shift((uint32_t)tb, (uint32_t)T, K);
            // t (T - t) does not fall before T / 2 and does not rise after it
            const bool mono = 2 * (int64_t)tb <= T || 2 * (int64_t)t >= T;
            int32_t id[kAcRun];
            if (mono && sa == se) {
#pragma unroll
                for (int e = 0; e < kAcRun; ++e) id[e] = ac_clamp((int64_t)(t + min(e, nv - 1)) + sg * (int64_t)sa, T);
            } else {
#pragma unroll
                for (int e = 0; e < kAcRun; ++e) id[e] = ac_index(t + min(e, nv - 1), T, K, sg);
            }
            uint32_t v[kAcRun];
            if (st) {
#pragma unroll
                for (int e = 0; e < kAcRun; ++e) {
                    const int64_t p = (int64_t)id[e] - wb;
                    PSS_DASSERT(p >= 0 && p < need);
                    v[e] = win[p];
                }
            } else {
#pragma unroll
                for (int e = 0; e < kAcRun; ++e) {
                    PSS_DASSERT(id[e] >= 0 && id[e] < T);
                    v[e] = row[id[e]];
                }
            }
            if (sub) {
#pragma unroll
                for (int e = 0; e < kAcRun; ++e) v[e] = __float_as_uint(__fsub_rn(__uint_as_float(v[e]), sb));
            }
            if (OVEC && nv == kAcRun) {
                *reinterpret_cast<uint4 *>(o + tl) = make_uint4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int e = 0; e < kAcRun; ++e)
                    if (e < nv) o[tl + e] = v[e];
            }
        }
    }
}

extern "C" {

int pss_accel_resample(const float *x, int32_t nser, int64_t T, int64_t ld, const int32_t *src, const int64_t *kappa,
                       const float *sub, int32_t nrows, int64_t n_out, float *out, int64_t out_ld, void *stream) {
    if (!x) return fail(PSS_EINVAL, "accel_resample: x is NULL");
    if (!src) return fail(PSS_EINVAL, "accel_resample: src is NULL");
    if (!kappa) return fail(PSS_EINVAL, "accel_resample: kappa is NULL");
    if (!out) return fail(PSS_EINVAL, "accel_resample: out is NULL");
    if (nser < 1) return fail(PSS_EINVAL, "accel_resample: nser %d < 1", nser);
    if (nrows < 1) return fail(PSS_EINVAL, "accel_resample: nrows %d < 1", nrows);
    if (T < 1) return fail(PSS_EINVAL, "accel_resample: T %lld < 1", (long long)T);
    if (T > (int64_t)0x7fffffff) return fail(PSS_EINVAL, "accel_resample: T %lld > 2^31 - 1", (long long)T);
    if (ld < T) return fail(PSS_EINVAL, "accel_resample: ld %lld < T %lld", (long long)ld, (long long)T);
    if (n_out < 1) return fail(PSS_EINVAL, "accel_resample: n_out %lld < 1", (long long)n_out);
    if (n_out > T) return fail(PSS_EINVAL, "accel_resample: n_out %lld > T %lld", (long long)n_out, (long long)T);
    if (out_ld < n_out)
        return fail(PSS_EINVAL, "accel_resample: out_ld %lld < n_out %lld", (long long)out_ld, (long long)n_out);
    const int64_t ngroups = ((int64_t)nrows + kAcNR - 1) / kAcNR;
    const int64_t ntiles = (n_out + kAcTB - 1) / kAcTB;
    const dim3 grid = grid_1d("accel_resample", ntiles, "time tiles", ngroups, "row groups");
    if (!grid.x) return PSS_EINVAL;
    AcArgs a;
    a.ld = ld; a.out_ld = out_ld; a.T = (int32_t)T; a.n_out = (int32_t)n_out; a.nser = nser; a.nrows = nrows;
    a.ngroups = (int32_t)ngroups; a.kmax = ((uint64_t)1 << 63) / (uint64_t)T;
    const uint32_t *xw = reinterpret_cast<const uint32_t *>(x);
    uint32_t *ow = reinterpret_cast<uint32_t *>(out);
    // 16-B stores need the output rows on the 16-B grid.  Same bits.
    if (on_grid16(out, out_ld))
        k_accel_resample<true><<<grid, dim3(kAcThreads), 0, (hipStream_t)stream>>>(xw, src, kappa, sub, ow, a);
    else
        k_accel_resample<false><<<grid, dim3(kAcThreads), 0, (hipStream_t)stream>>>(xw, src, kappa, sub, ow, a);
    LAUNCHCHK();
    return PSS_OK;
}

}  // extern "C"
