// pss_harmsum.hip -- periodicity search of the DM-time plane (extension, no
// reference counterpart): the incoherent harmonic sum of the power spectrum of
// every trial, summed from the top, normalised and reduced to one (z, level,
// bin) per cell of `cell` bins.  The definition (include/pss_hip.h:
// pss_harmonic_search), all in IEEE float32, one rounding per line, no fused
// multiply-add:
//
//   P[k]       = ((re_k re_k) + (im_k im_k)) scale[j]
//   idx(k,m,h) = (k m + h/2) / h                  (integers; <= k)
//   H_0 = P,   H_l[k] = H_{l-1}[k] + P[idx(k,1,h)] + P[idx(k,3,h)] + ...   (h = 2^l, odd m < h, rising)
//   z_l[k]     = (H_l[k] - h) a_l,   a_l = 2^(-l/2)
//   cell q     : lexicographic maximum of (z, -l, -k) over q cell <= k < (q + 1) cell,
//                k < nbin, idx(k,1,h) >= kmin.
//
//   k_harmonic_search<SRC> : a workgroup of 256 threads owns kHsTile = 2048 bins k
//       (the bin of the highest harmonic) of one trial.  Lanes run along k: thread i
//       owns k0 + i + 256 m, m < 8.  In sixteenths every term of every level is
//       idx = (k M + 8) >> 4 with M = m 16 / h in 1 .. 16, so a wave's 64 lanes
//       read at most 64 M / 16 + 1 consecutive elements per term.  The terms are
//       gathered through the vector cache; the 8 loads of a term are independent
//       and issued together.  Where they come from is the caller's choice:
//         * with a workspace (SRC = kHsPow): k_hs_power first writes the float32
//           powers P[j][k], kmin <= k < nbin, and the gathers read dwords.  A row
//           of powers is half a row of the spectrum and is computed once, not
//           once per term: at 16 harmonics this halves the time (DESIGN.md
//           section 9 has the same-box A/B);
//         * without one (work = NULL; SRC = kHsVec, 8-B loads when spec is on
//           the 8-B grid, or kHsElem, two dword loads -- the same values): the
//           terms are read straight from the spectrum and turned into power in
//           registers.  One harmonic reads every bin once, so there the extra
//           pass only costs.
//       The operations and their order are the same, so are the bits.  Nothing
//       is staged in LDS: the 16 windows of a 2048 tile would take 70 KB (2
//       workgroups per CU), and the gathers re-read lines that neighbouring
//       tiles of the same trial -- dealt to one XCD in runs -- have just pulled
//       into its L2.
//       A lane whose fundamental lies below kmin at level l skips the level's
//       loads (and every later level's: idx(k,1,h) falls with l), so no read
//       leaves [kmin, nbin) of the row.
//       A thread keeps the best (z, l) of each of its bins (strict >, l rising:
//       ties stay with the lower level; a NaN never compares greater).  The
//       cells are reduced as in pss_boxsearch.hip (cm_reduce_store,
//       pss_cellmax.hpp, shared by the two): (z, code) of the 2048 bins go
//       to LDS, thread i scans the bins 8 i .. 8 i + 7, then cell / 8
//       neighbouring threads combine by a butterfly of wave shuffles (and, for
//       cell >= 1024, across the waves through LDS) under the total order
//       "larger z, then smaller code" -- code = l << 16 | k - q cell.  One
//       thread per cell stores snr and code as dwords.  No atomics; the bits
//       depend on neither the alignment, the workspace nor the launch geometry.
#include "pss_cellmax.hpp"

using namespace pss;

static constexpr int kHsThreads = kCmThreads;
static constexpr int kHsOwn = kCmOwn;                     // bins per lane
static constexpr int kHsTile = kCmTile;                   // bins per workgroup
static constexpr int kHsMaxL = 5;                         // levels: 1, 2, 4, 8, 16 harmonics
static constexpr int64_t kHsMaxBin = (int64_t)1 << 27;    // k * 16 + 8 in 31 bits

struct HarmArgs {
    int64_t nbin, ld, out_ld, nq, ntiles, kmin;
    int32_t ndm, nl, cell, lcell;
};

// where the terms come from
enum : int { kHsElem = 0, kHsVec = 1, kHsPow = 2 };

// |X|^2 scale: two rounded products, one rounded sum, one rounded product
__device__ __forceinline__ float hs_norm(float re, float im, float scale) {
    return __fmul_rn(__fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im)), scale);
}

// P[idx] of the row: a row of the spectrum (SRC = kHsElem, kHsVec) or of the powers
template <int SRC>
__device__ __forceinline__ float hs_power(const float *row, int idx, float scale) {
    if (SRC == kHsPow) return row[idx];
    if (SRC == kHsVec) {
        const float2 v = reinterpret_cast<const float2 *>(row)[idx];
        return hs_norm(v.x, v.y, scale);
    }
    return hs_norm(row[2 * (int64_t)idx], row[2 * (int64_t)idx + 1], scale);
}

// the powers of the bins a sum can read, kmin <= k < nbin, of every trial -> work[j][k]
template <int SRC>
__global__ __launch_bounds__(kHsThreads) void k_hs_power(const float *__restrict__ spec,
                                                         const float *__restrict__ scale, float *__restrict__ work,
                                                         HarmArgs a) {
    const uint2 id = xcd_run_pair((unsigned)a.ntiles);     // (trial, tile) as k_harmonic_search
    const int j = (int)id.x;
    const int k0 = (int)id.y * kHsTile;
    PSS_DASSERT(j >= 0 && j < a.ndm && k0 < a.nbin);
    const float sc = scale[j];
    const float *row = spec + 2 * ((int64_t)j * a.ld);
    const int nbin = (int)a.nbin;
    const int kmin = (int)min(a.kmin, a.nbin);
#pragma unroll
    for (int i = 0; i < kHsOwn; ++i) {
        const int k = k0 + (int)threadIdx.x + i * kHsThreads;
        if (k >= kmin && k < nbin) work[(int64_t)j * a.nbin + k] = hs_power<SRC>(row, k, sc);
    }
}

template <int SRC>
__global__ __launch_bounds__(kHsThreads) void k_harmonic_search(const float *__restrict__ spec,
                                                                const float *__restrict__ scale,
                                                                float *__restrict__ snr, int32_t *__restrict__ code,
                                                                HarmArgs a) {
    __shared__ __align__(16) float wz[kHsTile];
    __shared__ __align__(16) int wcode[kHsTile];
    __shared__ float redz[kHsThreads / 64];
    __shared__ int redc[kHsThreads / 64];
    const int tid = threadIdx.x;
    PSS_DASSERT(a.nl >= 1 && a.nl <= kHsMaxL && a.kmin >= 1 && a.nbin <= kHsMaxBin);

    // workgroup id -> (trial, tile), tiles fastest, through the XCD run map
    const uint2 id = xcd_run_pair((unsigned)a.ntiles);
    const int j = (int)id.x;
    const int k0 = (int)id.y * kHsTile;
    PSS_DASSERT(j >= 0 && j < a.ndm && k0 < a.nbin);
    const float sc = scale[j];
    // (SRC = kHsPow: spec is the workspace, rows of nbin powers)
    const float *row = spec + (SRC == kHsPow ? (int64_t)j * a.nbin : 2 * ((int64_t)j * a.ld));
    const int nbin = (int)a.nbin;
    // a fundamental below kmin is invalid; kmin past the row leaves nothing valid
    const int kmin = (int)min(a.kmin, a.nbin);

    float H[kHsOwn], bz[kHsOwn];
    int bl[kHsOwn];
#pragma unroll
    for (int i = 0; i < kHsOwn; ++i) {
        H[i] = 0.0f;
        bz[i] = -INFINITY;
        bl[i] = 0;
    }
#pragma unroll
    for (int l = 0; l < kHsMaxL; ++l) {
        if (l < a.nl) {                                    // (wave-uniform)
            constexpr int kTop = 16;
            const int step = kTop >> l;                    // the fundamental in sixteenths of k
            bool ok[kHsOwn];
#pragma unroll
            for (int i = 0; i < kHsOwn; ++i) {
                const int k = k0 + tid + i * kHsThreads;
                // valid by index: k inside the row and the fundamental's bin at or above kmin
                ok[i] = k < nbin && ((k * step + 8) >> 4) >= kmin;
            }
            // the level's own terms: odd m < h, i.e. M = step, 3 step, 5 step, ...
#pragma unroll
            for (int M = step; M <= kTop; M += 2 * step) {
                float p[kHsOwn];
#pragma unroll
                for (int i = 0; i < kHsOwn; ++i) {
                    const int k = k0 + tid + i * kHsThreads;
                    const int idx = (k * M + 8) >> 4;
                    p[i] = 0.0f;
                    if (ok[i]) {
                        PSS_DASSERT(idx >= kmin && idx <= k && idx < nbin);
                        p[i] = hs_power<SRC>(row, idx, sc);
                    }
                }
#pragma unroll
                for (int i = 0; i < kHsOwn; ++i) H[i] = l == 0 ? p[i] : __fadd_rn(H[i], p[i]);
            }
            const float c = cm_coef(l);
            const float h = (float)(1 << l);
#pragma unroll
            for (int i = 0; i < kHsOwn; ++i) {
                const float z = __fmul_rn(__fsub_rn(H[i], h), c);
                if (ok[i] && z > bz[i]) {
                    bz[i] = z;
                    bl[i] = l;
                }
            }
        }
    }

    // per-cell reduction (pss_cellmax.hpp)
    cm_reduce_store(wz, wcode, redz, redc, bz, bl, tid, a.cell, a.lcell, (int64_t)(k0 >> a.lcell), a.nq, j, a.out_ld,
                    snr, code);
}

extern "C" {

int pss_harmonic_search(const float *spec, int32_t ndm, int64_t nbin, int64_t ld, const float *scale, int32_t nl,
                        int64_t kmin, int32_t cell, float *snr, int32_t *code, int64_t out_ld, float *work,
                        void *stream) {
    if (!spec) return fail(PSS_EINVAL, "harmonic_search: spec is NULL");
    if (!scale) return fail(PSS_EINVAL, "harmonic_search: scale is NULL");
    if (!snr) return fail(PSS_EINVAL, "harmonic_search: snr is NULL");
    if (!code) return fail(PSS_EINVAL, "harmonic_search: code is NULL");
    if (ndm < 1) return fail(PSS_EINVAL, "harmonic_search: ndm %d < 1", ndm);
    if (nbin < 1) return fail(PSS_EINVAL, "harmonic_search: nbin %lld < 1", (long long)nbin);
    if (nbin > kHsMaxBin)
        return fail(PSS_EINVAL, "harmonic_search: nbin %lld > 2^27 (16 k + 8 must fit 31 bits)", (long long)nbin);
    if (ld < nbin) return fail(PSS_EINVAL, "harmonic_search: ld %lld < nbin %lld", (long long)ld, (long long)nbin);
    if (nl < 1 || nl > kHsMaxL) return fail(PSS_EINVAL, "harmonic_search: nl %d outside [1, %d]", nl, kHsMaxL);
    if (kmin < 1) return fail(PSS_EINVAL, "harmonic_search: kmin %lld < 1", (long long)kmin);
    if (check_cell("harmonic_search", cell, kHsTile)) return PSS_EINVAL;
    const int64_t nq = (nbin - 1) / cell + 1;
    if (out_ld < nq) return fail(PSS_EINVAL, "harmonic_search: out_ld %lld < %lld cells", (long long)out_ld,
                                 (long long)nq);
    const int64_t ntiles = (nbin - 1) / kHsTile + 1;
    const dim3 grid = grid_1d("harmonic_search", ntiles, "bin tiles", ndm, "trials");
    if (!grid.x) return PSS_EINVAL;
    HarmArgs a;
    a.nbin = nbin; a.ld = ld; a.out_ld = out_ld; a.nq = nq; a.ntiles = ntiles; a.kmin = kmin;
    a.ndm = ndm; a.nl = nl; a.cell = cell;
    a.lcell = cell_log2(cell);
    hipStream_t st = (hipStream_t)stream;
    // 8-B loads of a complex element need the rows on the 8-B grid (a float pointer
    // promises 4).  Same bits.
    const bool vec = (uintptr_t)spec % 8 == 0;
    if (work) {
        if (vec)
            k_hs_power<kHsVec><<<grid, dim3(kHsThreads), 0, st>>>(spec, scale, work, a);
        else
            k_hs_power<kHsElem><<<grid, dim3(kHsThreads), 0, st>>>(spec, scale, work, a);
        LAUNCHCHK();
        k_harmonic_search<kHsPow><<<grid, dim3(kHsThreads), 0, st>>>(work, scale, snr, code, a);
    } else if (vec) {
        k_harmonic_search<kHsVec><<<grid, dim3(kHsThreads), 0, st>>>(spec, scale, snr, code, a);
    } else {
        k_harmonic_search<kHsElem><<<grid, dim3(kHsThreads), 0, st>>>(spec, scale, snr, code, a);
    }
    LAUNCHCHK();
    return PSS_OK;
}

}  // extern "C"
