// pss_boxsearch.hip -- single-pulse search of the DM-time plane (extension, no
// reference counterpart): a boxcar matched filter over the widths 2^k, k < nw,
// normalised per trial and reduced to one (S/N, width, time) per cell of `cell`
// start times.  The definition (include/pss_hip.h: pss_boxcar_search), all in
// IEEE float32, one rounding per line:
//
//   y[t]       = plane[j][t] - mean[j]
//   S_0        = y,   S_{k+1}[t] = S_k[t] + S_k[t + 2^k]        (balanced tree)
//   z_k[t]     = S_k[t] * (a_k * rstd[j]),   a_k = 2^(-k/2)
//   cell q     : lexicographic maximum of (z, -k, -t) over q cell <= t < (q+1) cell,
//                t + 2^k <= T.
//
//   k_boxcar_search<HB, VEC> : a workgroup of 256 threads owns kBsTile = 2048 start
//       times of one trial.  Lanes run along time: thread i holds the samples
//       t0 + i + 256 m, m < NI = 8 + HB, in registers -- its 8 own start times
//       and HB blocks of halo, 256 HB >= 2^(nw-1) - 1 (HB = 1 for nw <= 9, then
//       2, 4, 8, 16 for nw = 10 .. 13).  The row's window is staged in LDS once
//       (16-B loads when the row is on the 16-B grid, VEC, all issued before the
//       first LDS store; element loads otherwise -- the same values), the mean
//       subtracted as it is stored.  A level whose step 2^k is below 256 takes
//       its partner S_k[t + 2^k] from LDS (the level written there by every
//       thread, consecutive lanes on consecutive dwords: conflict-free); from
//       2^k = 256 on the partner is the thread's own register m + 2^k / 256 and
//       the levels need neither LDS nor a barrier.  That is the lever taken
//       against the halo: at nw = 13 the halo triples the adds (24 registers for
//       8 start times), but 4 of the 12 levels then cost one v_add per register
//       and nothing else.
//       Only the 8 own start times take the multiply and the compare; a sample
//       at or past T is staged as 0 and a candidate is valid by its index
//       (t + 2^k <= T), so no padding value ever reaches a result.  A thread
//       keeps the best (z, k) of each of its start times (strict >, k rising:
//       ties stay with the narrower width; a NaN never compares greater).
//       The cells (cm_reduce_store, pss_cellmax.hpp, shared with
//       pss_harmsum.hip): (z, code) of the 2048 start times go to LDS, thread i scans
//       the 8 consecutive times 8 i .. 8 i + 7 (one cell holds them all: cell is
//       a multiple of 16), then cell / 8 neighbouring threads combine by a
//       butterfly of wave shuffles (and, for cell >= 1024, across the waves
//       through LDS) under the total order "larger z, then smaller code" --
//       code = k << 16 | t - q cell, so a smaller code is the narrower width,
//       then the earlier time.  One thread per cell stores snr and code as
//       dwords; the cells of a tile are contiguous (cell <= 128: whole 64-B
//       segments).  No atomics, no workspace; the bits depend on neither the
//       alignment nor the launch geometry.
//       Logical workgroup index = trial * tiles + tile, dealt to the XCDs in
//       contiguous runs (as k_dedisperse): neighbouring tiles, which share a
//       halo, read it through one L2.
#include "pss_cellmax.hpp"

using namespace pss;

static constexpr int kBsThreads = kCmThreads;
static constexpr int kBsOwn = kCmOwn;                     // start times per lane
static constexpr int kBsTile = kCmTile;                   // start times per workgroup
static constexpr int kBsMaxW = 13;                        // widths 2^0 .. 2^12

struct BoxArgs {
    int64_t T, ld, out_ld, nq, ntiles;
    int32_t ndm, nw, cell, lcell;
};

// y[e] = row[e] - mean for e < valid = min(256 NI, samples left in the row),
// 0 for valid <= e < 256 (NI + 1) -> w[e]
template <int NI, bool VEC>
__device__ __forceinline__ void bs_stage(float *w, const float *row, int valid, float mean, int tid) {
    constexpr int kAll = kBsThreads * (NI + 1);           // floats of the window
    PSS_DASSERT(valid >= 1 && valid <= kBsThreads * NI);
    const int ng = (valid + 3) >> 2;                      // 16-B groups that hold a sample
    if (VEC && (valid & 3) == 0) {
        // every group whole and inside the row (all but a row's last tiles):
        // loads before stores, pinned, as stage_window (pss_window.hpp).
        // Lanes past the last group re-load it (in bounds) and store zeros.
        constexpr int NP = (kAll / 4 + kBsThreads - 1) / kBsThreads;
        const float4 *src = reinterpret_cast<const float4 *>(row);
        float4 v[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) v[i] = src[min(tid + i * kBsThreads, ng - 1)];
#pragma unroll
        for (int i = 0; i < NP; ++i) asm volatile("" : "+v"(v[i].x), "+v"(v[i].y), "+v"(v[i].z), "+v"(v[i].w));
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const int g = tid + i * kBsThreads;
            if (g < kAll / 4) {
                float4 y = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (g < ng) {
                    y.x = v[i].x - mean;
                    y.y = v[i].y - mean;
                    y.z = v[i].z - mean;
                    y.w = v[i].w - mean;
                }
                *reinterpret_cast<float4 *>(w + 4 * g) = y;
            }
        }
        return;
    }
    float x[NI + 1];
#pragma unroll
    for (int i = 0; i <= NI; ++i) {
        const int e = tid + i * kBsThreads;
        x[i] = e < valid ? row[e] : mean;
    }
#pragma unroll
    for (int i = 0; i <= NI; ++i) {
        const int e = tid + i * kBsThreads;
        const float y = x[i] - mean;
        w[e] = e < valid ? y : 0.0f;
    }
}

template <int HB, bool VEC>
__global__ __launch_bounds__(kBsThreads) void k_boxcar_search(const float *__restrict__ plane,
                                                              const float *__restrict__ mean,
                                                              const float *__restrict__ rstd,
                                                              float *__restrict__ snr, int32_t *__restrict__ code,
                                                              BoxArgs a) {
    constexpr int NI = kBsOwn + HB;                       // registers of samples per lane
    // levels: HB == 1 serves every nw <= 9 (all steps below 256, nw at run
    // time); a larger HB serves exactly one nw
    constexpr int kNW = HB == 1 ? 9 : HB == 2 ? 10 : HB == 4 ? 11 : HB == 8 ? 12 : 13;
    static_assert(kBsThreads * HB >= (1 << (kNW - 1)) - 1, "the halo blocks hold the widest box");
    constexpr int kWin = kBsThreads * (NI + 1) > 2 * kBsTile ? kBsThreads * (NI + 1) : 2 * kBsTile;
    __shared__ __align__(16) float win[kWin];
    __shared__ float redz[kBsThreads / 64];
    __shared__ int redc[kBsThreads / 64];
    const int tid = threadIdx.x;
    const int nw = HB == 1 ? a.nw : kNW;
    PSS_DASSERT(a.nw >= 1 && a.nw <= kNW && (HB == 1 || a.nw == kNW));

    // workgroup id -> (trial, tile), tiles fastest, through the XCD run map
    const uint2 id = xcd_run_pair((unsigned)a.ntiles);
    const int j = (int)id.x;
    const int64_t t0 = (int64_t)id.y * kBsTile;
    PSS_DASSERT(j >= 0 && j < a.ndm && t0 < a.T);
    const float mu = mean[j];
    const float rs = rstd[j];
    const int64_t left = a.T - t0;                         // samples of the row from t0 on (>= 1)
    // the window: NI blocks, which hold the tile's boxes (2048 + 2^(nw-1) - 1 samples)
    const int valid = (int)min((int64_t)(kBsThreads * NI), left);
    const int lim = (int)min((int64_t)(2 * kBsTile + (1 << kBsMaxW)), left);   // `left` in 32 bits

    bs_stage<NI, VEC>(win, plane + (int64_t)j * a.ld + t0, valid, mu, tid);
    __syncthreads();
    float S[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) S[i] = win[tid + i * kBsThreads];

    float bz[kBsOwn];
    int bk[kBsOwn];
#pragma unroll
    for (int i = 0; i < kBsOwn; ++i) {
        bz[i] = -INFINITY;
        bk[i] = 0;
    }
#pragma unroll
    for (int k = 0; k < kNW; ++k) {
        if (k < nw) {                                      // (wave-uniform)
            const float c = cm_coef(k) * rs;
#pragma unroll
            for (int i = 0; i < kBsOwn; ++i) {
                const float z = S[i] * c;
                // valid by index: the box [t, t + 2^k) inside [0, T)
                const bool ok = tid + i * kBsThreads + (1 << k) <= lim;
                if (ok && z > bz[i]) {
                    bz[i] = z;
                    bk[i] = k;
                }
            }
            if (k + 1 < nw) {
                constexpr int kStepMax = kBsThreads;
                const int h = 1 << k;
                if (h < kStepMax) {
                    if (k > 0) {
                        __syncthreads();                   // the previous level's reads are done
#pragma unroll
                        for (int i = 0; i < NI; ++i) win[tid + i * kBsThreads] = S[i];
                        __syncthreads();
                    }
                    // (the last block's partners past the window's NI blocks are
                    // the zero block: sums no valid candidate depends on)
#pragma unroll
                    for (int i = 0; i < NI; ++i) {
                        PSS_DASSERT(tid + h + i * kBsThreads < kBsThreads * (NI + 1));
                        const float b = win[tid + h + i * kBsThreads];
                        S[i] = S[i] + b;
                    }
                } else {
                    const int m = h / kStepMax;            // own registers, rising i: S[i + m] is still level k
#pragma unroll
                    for (int i = 0; i < NI; ++i)
                        if (i + m < NI) S[i] = S[i] + S[i + m];
                }
            }
        }
    }

    // per-cell reduction (pss_cellmax.hpp): the window is free once every thread has read its partners
    __syncthreads();
    cm_reduce_store(win, reinterpret_cast<int *>(win + kBsTile), redz, redc, bz, bk, tid, a.cell, a.lcell,
                    t0 >> a.lcell, a.nq, j, a.out_ld, snr, code);
}

template <int HB>
static int bs_launch(const float *plane, const float *mean, const float *rstd, float *snr, int32_t *code,
                     const BoxArgs &a, dim3 grid, hipStream_t st) {
    // 16-B loads of the window need the rows on the 16-B grid.  Same bits.
    if (on_grid16(plane, a.ld))
        k_boxcar_search<HB, true><<<grid, dim3(kBsThreads), 0, st>>>(plane, mean, rstd, snr, code, a);
    else
        k_boxcar_search<HB, false><<<grid, dim3(kBsThreads), 0, st>>>(plane, mean, rstd, snr, code, a);
    LAUNCHCHK();
    return PSS_OK;
}

extern "C" {

int pss_boxcar_search(const float *plane, int32_t ndm, int64_t T, int64_t ld, const float *mean, const float *rstd,
                      int32_t nw, int32_t cell, float *snr, int32_t *code, int64_t out_ld, void *stream) {
    if (!plane) return fail(PSS_EINVAL, "boxcar_search: plane is NULL");
    if (!mean) return fail(PSS_EINVAL, "boxcar_search: mean is NULL");
    if (!rstd) return fail(PSS_EINVAL, "boxcar_search: rstd is NULL");
    if (!snr) return fail(PSS_EINVAL, "boxcar_search: snr is NULL");
    if (!code) return fail(PSS_EINVAL, "boxcar_search: code is NULL");
    if (ndm < 1) return fail(PSS_EINVAL, "boxcar_search: ndm %d < 1", ndm);
    if (T < 1) return fail(PSS_EINVAL, "boxcar_search: T %lld < 1", (long long)T);
    if (ld < T) return fail(PSS_EINVAL, "boxcar_search: ld %lld < T %lld", (long long)ld, (long long)T);
    if (nw < 1 || nw > kBsMaxW) return fail(PSS_EINVAL, "boxcar_search: nw %d outside [1, %d]", nw, kBsMaxW);
    if (check_cell("boxcar_search", cell, kBsTile)) return PSS_EINVAL;
    const int64_t nq = (T - 1) / cell + 1;
    if (out_ld < nq) return fail(PSS_EINVAL, "boxcar_search: out_ld %lld < %lld cells", (long long)out_ld,
                                 (long long)nq);
    const int64_t ntiles = (T - 1) / kBsTile + 1;
    const dim3 grid = grid_1d("boxcar_search", ntiles, "time tiles", ndm, "trials");
    if (!grid.x) return PSS_EINVAL;
    BoxArgs a;
    a.T = T; a.ld = ld; a.out_ld = out_ld; a.nq = nq; a.ntiles = ntiles;
    a.ndm = ndm; a.nw = nw; a.cell = cell;
    a.lcell = cell_log2(cell);
    hipStream_t st = (hipStream_t)stream;
    switch (nw) {
        case 13: return bs_launch<16>(plane, mean, rstd, snr, code, a, grid, st);
        case 12: return bs_launch<8>(plane, mean, rstd, snr, code, a, grid, st);
        case 11: return bs_launch<4>(plane, mean, rstd, snr, code, a, grid, st);
        case 10: return bs_launch<2>(plane, mean, rstd, snr, code, a, grid, st);
        default: return bs_launch<1>(plane, mean, rstd, snr, code, a, grid, st);
    }
}

}  // extern "C"
