// pss_whiten.hip -- whitening of a power spectrum between the transform and
// the harmonic sums (extension, no reference counterpart): the lower median of
// the power over ragged blocks of bins, then every bin divided by a median
// interpolated between block centres, known interference lines replaced by a
// neutral value (include/pss_hip.h has the definitions).  Two kernels, because
// a bin's norm needs the medians of both its neighbours' blocks and the
// whitening may run in place: a fused kernel would read a block that a
// neighbouring workgroup is rewriting.
//
//   k_spectrum_medians<ALN8> : a wave owns a block of w <= 256 bins; a
//       workgroup of 4 waves owns kMdPerWg = 32 consecutive blocks of one
//       trial, its waves taking neighbouring blocks at any one time, so that
//       the workgroup reads one contiguous stretch of the row.  Lane l holds
//       the keys of the bins e + l + 64 i, i < KPL (KPL = 1, 2 or 4 by the
//       block's width: 64 lanes x 8 B a load, ALN8; two dword loads per bin
//       where the rows are off the 8-B grid).  Selection finds the 32 key
//       bits of the median from the top: with the bits found so far and the
//       next one set as a threshold t, the key at the rank reaches t iff at
//       most rank keys lie below t -- one vector compare of the key with a
//       scalar per i, a population count of its lane mask, a scalar compare.
//       It is the scalar unit that bounds the kernel (one instruction a SIMD
//       every four cycles), so the per-bit work there is kept to six
//       instructions at KPL = 2; no mask of candidates is carried along.  A
//       selection is exact: the bits are those of the sort.
//   k_spectrum_whiten<VW> : a workgroup of 256 threads owns kWtTile = 1024
//       bins of one trial.  It finds the blocks whose centres bracket its bins
//       by two binary searches in the table (wave-uniform), copies their
//       doubled centres (relative to the tile, 32 bits) and medians to LDS --
//       at most kWtTile + 2 of them, because doubled centres of a valid table
//       rise by at least 2 -- and every bin finds its pair there by a short
//       binary search.  VW = 4: a thread moves two bins per 16-B load and
//       store, from the tile's first bin on the 16-B grid on (a row of spec and
//       its row of out sit alike on that grid; a bin before it goes alone);
//       VW = 2: 8-B accesses; VW = 1: dwords.  The same bits by every route.
//   Either kernel clamps what it takes from the table, so that no read leaves
//   a row and no LDS index its array whatever the table holds.  Logical
//   workgroup index = trial * (groups of a trial) + group, dealt to the XCDs in
//   contiguous runs.  No atomics, no workspace.
#include "pss_common.hpp"

using namespace pss;

static constexpr int kMdThreads = 256;
static constexpr int kMdWaves = kMdThreads / 64;
static constexpr int kMdMaxW = 256;                       // the widest block a wave selects from
static constexpr int kMdRun = 8;                          // blocks per wave
static constexpr int kMdPerWg = kMdWaves * kMdRun;        // blocks per workgroup (32)
static constexpr int kWtThreads = 256;
static constexpr int kWtTile = 1024;                      // bins per workgroup
static constexpr int kWtCap = kWtTile + 2;                // staged block centres
static constexpr uint32_t kLn2Bits = 0x3F317218u;         // float32(ln 2)
static constexpr uint32_t kNanKey = 0xFFFFFFFFu, kNanBits = 0x7FC00000u;

struct WhArgs {
    int64_t nbin, ld, out_ld, med_ld;
    int32_t nblk, ngroups;                                // blocks; workgroups per trial
};

// key(P) of bin k of a row: (re re) + (im im), every operation rounded once
template <bool ALN8>
__device__ __forceinline__ uint32_t md_key(const float *__restrict__ row, int64_t k) {
    float re, im;
    if (ALN8) {
        const float2 v = reinterpret_cast<const float2 *>(row)[k];
        re = v.x;
        im = v.y;
    } else {
        re = row[2 * k];
        im = row[2 * k + 1];
    }
    const float rr = re * re;
    const float ii = im * im;
    const float p = rr + ii;
    return p != p ? kNanKey : __float_as_uint(p);
}

// the key at sorted index (w - 1) / 2 of the w keys of the block [e, e + w),
// 1 <= w <= 64 KPL: the same value in every lane
template <int KPL, bool ALN8>
__device__ __forceinline__ uint32_t md_select(const float *__restrict__ row, int64_t e, int w, int lane) {
    uint32_t key[KPL];
#pragma unroll
    for (int i = 0; i < KPL; ++i) {
        const int p = lane + 64 * i;
        const uint32_t k = md_key<ALN8>(row, e + min(p, w - 1));   // (a lane past the block repeats its last bin,
        key[i] = p < w ? k : kNanKey;                              // and sorts behind every bin of the block)
        // (the key in a register of its own: otherwise its tests are folded
        // into every one of the 32 compares below)
        asm volatile("" : "+v"(key[i]));
    }
    const int rank = (w - 1) >> 1;
    uint32_t med = 0;
    for (int bit = 31; bit >= 0; --bit) {
        // the key at the rank reaches t iff at most rank keys lie below t
        const uint32_t t = med | (1u << bit);
        int below = 0;
#pragma unroll
        for (int i = 0; i < KPL; ++i) below += __popcll(__builtin_amdgcn_ballot_w64(key[i] < t));
        if (below <= rank) med = t;
    }
    return med;
}

template <bool ALN8>
__global__ __launch_bounds__(kMdThreads) void k_spectrum_medians(const float *__restrict__ spec,
                                                                 const int64_t *__restrict__ edges,
                                                                 uint32_t *__restrict__ med, WhArgs a) {
    const uint2 id = xcd_run_pair((unsigned)a.ngroups);
    const int64_t j = id.x;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = threadIdx.x & 63;
    const float *row = spec + 2 * j * a.ld;
    const int b0 = (int)id.y * kMdPerWg;
    for (int r = 0; r < kMdRun; ++r) {
        const int b = b0 + r * kMdWaves + wave;
        if (b >= a.nblk) break;
        // [e, e + w) inside the row, w <= 256, whatever the table holds
        const int64_t e = min(max(edges[b], (int64_t)0), a.nbin);
        const int w = (int)(min(max(edges[b + 1], e), min(e + kMdMaxW, a.nbin)) - e);
        uint32_t m = kNanKey;                              // (w = 0: only a table that is not valid)
        if (w > 128)
            m = md_select<4, ALN8>(row, e, w, lane);
        else if (w > 64)
            m = md_select<2, ALN8>(row, e, w, lane);
        else if (w > 0)
            m = md_select<1, ALN8>(row, e, w, lane);
        if (lane == 0) med[j * a.med_ld + b] = m == kNanKey ? kNanBits : m;
    }
}

// the doubled centre of block b
__device__ __forceinline__ int64_t wt_centre(const int64_t *__restrict__ edges, int b) {
    return edges[b] + edges[b + 1] - 1;
}

// the first b in [lo, hi) with d_b > x, hi if none
__device__ __forceinline__ int wt_upper(const int64_t *__restrict__ edges, int lo, int hi, int64_t x) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (wt_centre(edges, mid) <= x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// one bin: (re, im) of bin k, local doubled offset x = 2 (k - k0), through the staged tables
__device__ __forceinline__ float2 wt_bin(float re, float im, int64_t k, int x, const int32_t *sd, const float *sm, int cnt,
                                         int64_t e0, const uint8_t *__restrict__ zap) {
    if (k < e0) return make_float2(0.0f, 0.0f);
    if (zap && zap[k]) return make_float2(1.0f, 0.0f);
    int lo = 0, hi = cnt;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sd[mid] <= x)
            lo = mid + 1;
        else
            hi = mid;
    }
    const int p = lo - 1;                                 // the last staged centre at or below the bin
    float norm;
    if (p < 0) {
        norm = sm[0];
    } else if (p == cnt - 1) {
        norm = sm[cnt - 1];
    } else {
        const float num = (float)(x - sd[p]);
        const float den = (float)(sd[p + 1] - sd[p]);
        const float f = num / den;
        const float diff = sm[p + 1] - sm[p];
        const float t = diff * f;
        norm = sm[p] + t;
    }
    const float q = __uint_as_float(kLn2Bits) / norm;
    const float s = (norm > 0.0f && norm < __uint_as_float(0x7F800000u)) ? sqrtf(q) : 0.0f;
    const float ore = re * s;
    const float oim = im * s;
    return make_float2(ore, oim);
}

template <int VW>
__global__ __launch_bounds__(kWtThreads) void k_spectrum_whiten(const float *spec, const int64_t *__restrict__ edges,
                                                                const float *__restrict__ med,
                                                                const uint8_t *__restrict__ zap, float *out, WhArgs a) {
    __shared__ int32_t sd[kWtCap];
    __shared__ float sm[kWtCap];
    const int tid = threadIdx.x;
    const uint2 id = xcd_run_pair((unsigned)a.ngroups);
    const int64_t j = id.x;
    const int64_t k0 = (int64_t)id.y * kWtTile;
    const int len = (int)min((int64_t)kWtTile, a.nbin - k0);
    PSS_DASSERT(len >= 1);
    // the blocks whose centres bracket the tile: from the last centre at or
    // below its first bin (block 0 if none) to the first centre above its last
    // bin (the last block if none)
    const int ub = wt_upper(edges, 0, a.nblk, 2 * k0);
    const int bl = max(ub - 1, 0);
    const int bh = min(wt_upper(edges, bl, a.nblk, 2 * (k0 + len - 1)), a.nblk - 1);
    const int cnt = min(bh - bl + 1, kWtCap);             // (the cap: only a table that is not valid)
    PSS_DASSERT(cnt >= 1);
    for (int i = tid; i < cnt; i += kWtThreads) {
        const int64_t d = wt_centre(edges, bl + i) - 2 * k0;
        sd[i] = (int32_t)min(max(d, -(int64_t)(1 << 30)), (int64_t)(1 << 30));
        sm[i] = med[j * a.med_ld + bl + i];
    }
    __syncthreads();
    const int64_t e0 = edges[0];
    const float *row = spec + 2 * (j * a.ld + k0);
    float *orow = out + 2 * (j * a.out_ld + k0);
    if (VW == 4) {
        // bin ph of the tile is its first on the 16-B grid, in spec and in out
        // alike (the launcher's condition); a bin before it goes alone
        const int ph = (int)(((uintptr_t)row >> 3) & 1);
        if (ph && tid == kWtThreads - 1) {
            const float2 v = *reinterpret_cast<const float2 *>(row);
            *reinterpret_cast<float2 *>(orow) = wt_bin(v.x, v.y, k0, 0, sd, sm, cnt, e0, zap);
        }
#pragma unroll
        for (int i = 0; i < kWtTile / (2 * kWtThreads); ++i) {
            const int r = ph + 2 * (tid + i * kWtThreads);
            if (r + 1 < len) {
                const float4 v = *reinterpret_cast<const float4 *>(row + 2 * r);
                const float2 o0 = wt_bin(v.x, v.y, k0 + r, 2 * r, sd, sm, cnt, e0, zap);
                const float2 o1 = wt_bin(v.z, v.w, k0 + r + 1, 2 * r + 2, sd, sm, cnt, e0, zap);
                *reinterpret_cast<float4 *>(orow + 2 * r) = make_float4(o0.x, o0.y, o1.x, o1.y);
            } else if (r < len) {
                const float2 v = *reinterpret_cast<const float2 *>(row + 2 * r);
                *reinterpret_cast<float2 *>(orow + 2 * r) = wt_bin(v.x, v.y, k0 + r, 2 * r, sd, sm, cnt, e0, zap);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < kWtTile / kWtThreads; ++i) {
            const int r = tid + i * kWtThreads;
            if (r >= len) continue;
            if (VW == 2) {
                const float2 v = *reinterpret_cast<const float2 *>(row + 2 * r);
                *reinterpret_cast<float2 *>(orow + 2 * r) = wt_bin(v.x, v.y, k0 + r, 2 * r, sd, sm, cnt, e0, zap);
            } else {
                const float re = row[2 * r];
                const float im = row[2 * r + 1];
                const float2 o = wt_bin(re, im, k0 + r, 2 * r, sd, sm, cnt, e0, zap);
                orow[2 * r] = o.x;
                orow[2 * r + 1] = o.y;
            }
        }
    }
}

// what the two entry points check alike
static int wh_check(const char *what, const float *spec, int32_t ndm, int64_t nbin, int64_t ld, const int64_t *edges,
                    int32_t nblk, const float *med, int64_t med_ld) {
    if (!spec) return fail(PSS_EINVAL, "%s: spec is NULL", what);
    if (!edges) return fail(PSS_EINVAL, "%s: edges is NULL", what);
    if (!med) return fail(PSS_EINVAL, "%s: med is NULL", what);
    if (ndm < 1) return fail(PSS_EINVAL, "%s: ndm %d < 1", what, ndm);
    if (nbin < 1) return fail(PSS_EINVAL, "%s: nbin %lld < 1", what, (long long)nbin);
    if (nblk < 1) return fail(PSS_EINVAL, "%s: nblk %d < 1", what, nblk);
    if (nblk > nbin) return fail(PSS_EINVAL, "%s: nblk %d > nbin %lld", what, nblk, (long long)nbin);
    if (ld < nbin) return fail(PSS_EINVAL, "%s: ld %lld < nbin %lld", what, (long long)ld, (long long)nbin);
    if (med_ld < nblk) return fail(PSS_EINVAL, "%s: med_ld %lld < nblk %d", what, (long long)med_ld, nblk);
    return PSS_OK;
}

extern "C" {

int pss_spectrum_medians(const float *spec, int32_t ndm, int64_t nbin, int64_t ld, const int64_t *edges, int32_t nblk,
                         float *med, int64_t med_ld, void *stream) {
    if (wh_check("spectrum_medians", spec, ndm, nbin, ld, edges, nblk, med, med_ld)) return PSS_EINVAL;
    const int64_t ngroups = ((int64_t)nblk - 1) / kMdPerWg + 1;
    const dim3 grid = grid_1d("spectrum_medians", ngroups, "block groups", ndm, "trials");
    if (!grid.x) return PSS_EINVAL;
    WhArgs a;
    a.nbin = nbin; a.ld = ld; a.out_ld = 0; a.med_ld = med_ld; a.nblk = nblk; a.ngroups = (int32_t)ngroups;
    uint32_t *mw = reinterpret_cast<uint32_t *>(med);
    // 8-B loads of a complex element need the rows on the 8-B grid (a float pointer
    // promises 4).  Same bits.
    if ((uintptr_t)spec % 8 == 0)
        k_spectrum_medians<true><<<grid, dim3(kMdThreads), 0, (hipStream_t)stream>>>(spec, edges, mw, a);
    else
        k_spectrum_medians<false><<<grid, dim3(kMdThreads), 0, (hipStream_t)stream>>>(spec, edges, mw, a);
    LAUNCHCHK();
    return PSS_OK;
}

int pss_spectrum_whiten(const float *spec, int32_t ndm, int64_t nbin, int64_t ld, const int64_t *edges, int32_t nblk,
                        const float *med, int64_t med_ld, const uint8_t *zap, float *out, int64_t out_ld,
                        void *stream) {
    if (wh_check("spectrum_whiten", spec, ndm, nbin, ld, edges, nblk, med, med_ld)) return PSS_EINVAL;
    if (!out) return fail(PSS_EINVAL, "spectrum_whiten: out is NULL");
    if (out_ld < nbin)
        return fail(PSS_EINVAL, "spectrum_whiten: out_ld %lld < nbin %lld", (long long)out_ld, (long long)nbin);
    if (!(out == spec && out_ld == ld)) {
        // bytes [lo, hi) of either: (ndm - 1) rows and the bins of the last
        const uintptr_t s_lo = (uintptr_t)spec, s_hi = s_lo + (uintptr_t)(((int64_t)(ndm - 1) * ld + nbin) * 8);
        const uintptr_t o_lo = (uintptr_t)out, o_hi = o_lo + (uintptr_t)(((int64_t)(ndm - 1) * out_ld + nbin) * 8);
        if (s_lo < o_hi && o_lo < s_hi)
            return fail(PSS_EINVAL, "spectrum_whiten: out overlaps spec without being spec itself (in place: out == "
                                    "spec and out_ld == ld)");
    }
    const int64_t ngroups = (nbin - 1) / kWtTile + 1;
    const dim3 grid = grid_1d("spectrum_whiten", ngroups, "bin tiles", ndm, "trials");
    if (!grid.x) return PSS_EINVAL;
    WhArgs a;
    a.nbin = nbin; a.ld = ld; a.out_ld = out_ld; a.med_ld = med_ld; a.nblk = nblk; a.ngroups = (int32_t)ngroups;
    hipStream_t st = (hipStream_t)stream;
    // 8-B accesses need both on the 8-B grid (a float pointer promises 4);
    // 16-B accesses, two complex elements, also every row of out at the
    // position on the 16-B grid that the row of spec has (in place: always; a
    // transform's nbin + 1 elements per row put every other row off that grid,
    // which the kernel takes per row).  Same bits.
    const bool v8 = (uintptr_t)spec % 8 == 0 && (uintptr_t)out % 8 == 0;
    const bool v16 = v8 && (((uintptr_t)spec ^ (uintptr_t)out) & 8) == 0 && (ld - out_ld) % 2 == 0;
    if (v16)
        k_spectrum_whiten<4><<<grid, dim3(kWtThreads), 0, st>>>(spec, edges, med, zap, out, a);
    else if (v8)
        k_spectrum_whiten<2><<<grid, dim3(kWtThreads), 0, st>>>(spec, edges, med, zap, out, a);
    else
        k_spectrum_whiten<1><<<grid, dim3(kWtThreads), 0, st>>>(spec, edges, med, zap, out, a);
    LAUNCHCHK();
    return PSS_OK;
}

}  // extern "C"
