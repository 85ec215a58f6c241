// pss_dedisperse.hip -- incoherent dedispersion over trial DMs (extension, no
// reference counterpart): the DM-time plane of a [chan][time] filterbank,
//
//   out[j][t] = sum_{c < nchan} data[c][t + d(j, c)],   t < T = n - max_delay,
//
// the exact direct sum over an arbitrary integer delay table d[ndm][nchan]
// (clamped to [0, max_delay] as it is loaded).
//
//   k_dedisperse<VEC> : a workgroup of 256 threads owns kTB = 2048 output times
//       of kND = 8 neighbouring trials and walks the channels in order, kCB = 2
//       per barrier pair.  Lanes run along time: thread i holds times
//       t0 + i + 256 k (k < 8) of each of its trials, 64 accumulators.
//       Per channel c, with dmin / dmax the extreme delays of the workgroup's
//       trials (wave-uniform, scalar loads of the table):
//         staged  (dmax - dmin <= kSpread = 2044): the window
//                 data[c][ws .. t0 + dmax + 2048), ws = (t0 + dmin) & ~3, is
//                 copied to LDS once (stage_window, pss_window.hpp: 16-B
//                 loads when the row is on the 16-B grid, VEC; dwords
//                 otherwise -- the same values) and every
//                 trial reads its 8 samples per lane from it at the uniform
//                 offset t0 + d - ws: consecutive lanes read consecutive
//                 dwords, conflict-free at any offset.  The channel's row is
//                 read from global memory once per 8 trials.
//         wide    (a wider spread): the general path.  The trials take turns,
//                 two at a time: each copies its own samples
//                 data[c][t0 + d .. + 2048) into half of the channel's LDS
//                 buffer (dword loads), between two barriers, and reads them
//                 back the same way -- one global read of the row per trial.
//       Either way a sample joins its accumulator as `acc += x` in increasing
//       c, so the bits of out[j][t] depend on neither the path, the alignment
//       nor the launch geometry.  No atomics, no workspace.
//       The finished tile goes to out[j][t0 ..] as dword stores, 256 B per
//       wave-instruction.
//       Logical workgroup index = time tile * (trial groups) + trial group,
//       dealt to the XCDs in contiguous runs: the groups of one time tile run
//       together on one XCD and share its rows in that L2.
//
//   k_dedisperse_banded<VEC> : the same tile (dd_tile, shared) summed over one
//       band of channels only, read from one of several source planes:
//
//         out[j * nb + s][t] = sum_{c in band s} src(j)[c][t + d(j, c)],
//
//       nb = ceil(nchan / band), src(j) = min(j / per_src, nsrc - 1).  Both
//       stages of the sub-band dedispersion (telescope/subband.py) are calls of
//       it.  The trials are cut into groups of 8 inside each source (per_src =
//       5: groups of 5, 5, ..), so a workgroup reads one source.  Logical
//       workgroup index = (time tile * nb + band) * (trial groups) + trial
//       group, through the same run map: the bands and groups of one time tile
//       run on one XCD.  With one source and one band it is k_dedisperse's
//       sum, operation for operation.
#include <algorithm>

#include "pss_common.hpp"
#include "pss_window.hpp"

using namespace pss;

static constexpr int kDdThreads = 256;
static constexpr int kDdS = 8;                        // samples per lane and trial
static constexpr int kTB = kDdThreads * kDdS;         // output times per workgroup
static constexpr int kND = 8;                         // trials per workgroup
// channels per barrier pair, and trials whose LDS reads are in flight together
static constexpr int kCB = 2;
static constexpr int kNJ = 2;
static constexpr int kWin = 2 * kTB;                  // staged window, floats per channel
static_assert(kNJ * kTB <= kWin && kND % kNJ == 0, "the wide path's trials share the window");
static constexpr int kSpread = kWin - kTB - 4;        // widest staged spread of a channel's delays

struct DdArgs {
    int64_t n, ld, out_ld, T;
    int32_t nchan, ndm, max_delay, ngroups;
};

// acc[i][k] += w[off[i] + tid + 256 k] for NJ trials: off <= kWin - kTB, so the
// reads stay inside the window whatever the tile's length (a short tile's lanes
// past `len` add stale LDS words to accumulators that are never stored)
template <int NJ>
__device__ __forceinline__ void dd_accum(float (*acc)[kDdS], const float *w, const int (&off)[NJ], int tid) {
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        PSS_DASSERT(off[i] >= 0 && off[i] + kTB <= kWin);
        const float *p = w + off[i] + tid;
#pragma unroll
        for (int k = 0; k < kDdS; ++k) acc[i][k] += p[k * kDdThreads];
    }
    // NJ trials' reads (8 each) in flight at a time: the sums are pinned here (an
    // empty asm that "modifies" them) and nothing is scheduled across.
    // Otherwise the adds sink below the following trials' reads, 64 loaded
    // values stay live beside the 64 accumulators, and two waves per SIMD are
    // lost (144 registers)
#pragma unroll
    for (int i = 0; i < NJ; ++i)
#pragma unroll
        for (int k = 0; k < kDdS; ++k) asm volatile("" : "+v"(acc[i][k]));
    __builtin_amdgcn_sched_barrier(0);
}

// One workgroup's tile: times t0 .. t0 + len (len <= kTB) of the nd <= kND trials
// j0 .. (rows of `tab`, ntab entries each), summed over the channels
// [c_lo, c_hi) of data[c][ld] in increasing c; trial j0 + j goes to o0 + j * orow.
template <bool VEC>
__device__ __forceinline__ void dd_tile(float (*win)[kWin], const float *__restrict__ data,
                                        const int32_t *__restrict__ tab, float *__restrict__ o0, int64_t orow,
                                        int c_lo, int c_hi, int ntab, int j0, int nd, int64_t t0, int len, int64_t n,
                                        int64_t ld, int max_delay, int tid) {
    float acc[kND][kDdS];
#pragma unroll
    for (int j = 0; j < kND; ++j)
#pragma unroll
        for (int k = 0; k < kDdS; ++k) acc[j][k] = 0.0f;

    for (int c0 = c_lo; c0 < c_hi; c0 += kCB) {
        int d[kCB][kND];
        int64_t ws[kCB];
        bool staged[kCB];
#pragma unroll
        for (int cb = 0; cb < kCB; ++cb) {
            const int c = c0 + cb;
            staged[cb] = false;
            ws[cb] = 0;
            if (c >= c_hi) continue;
            int dmin = max_delay, dmax = 0;
#pragma unroll
            for (int j = 0; j < kND; ++j) {
                // (a ragged group repeats its last trial: summed, never stored)
                const int jj = j0 + min(j, nd - 1);
                d[cb][j] = min(max(tab[(int64_t)jj * ntab + c], 0), max_delay);
                dmin = min(dmin, d[cb][j]);
                dmax = max(dmax, d[cb][j]);
            }
            if (dmax - dmin > kSpread) continue;
            staged[cb] = true;
            ws[cb] = (t0 + dmin) & ~(int64_t)3;
            // the window's last needed sample is t0 + len - 1 + dmax <= n - 1
            const int need = (int)(t0 + dmax - ws[cb]) + len;  // <= 3 + kSpread + kTB < kWin
            // (samples at or past n, never needed, are zeros; ws >= 0: no HEAD)
            stage_window<kDdThreads, kWin, VEC, false>(win[cb], data + (int64_t)c * ld, ws[cb], need, n, tid);
        }
        __syncthreads();
#pragma unroll
        for (int cb = 0; cb < kCB; ++cb) {
            const int c = c0 + cb;
            if (c >= c_hi) continue;
            // (one accumulate serves both paths: an if / else around two copies of
            // it joins the 64 accumulators in phis that cost 60 more registers)
            const float *row = data + (int64_t)c * ld + t0;
#pragma unroll
            for (int j = 0; j < kND; j += kNJ) {
                int off[kNJ];
#pragma unroll
                for (int i = 0; i < kNJ; ++i) off[i] = staged[cb] ? (int)(t0 + d[cb][j + i] - ws[cb]) : i * kTB;
                if (!staged[cb]) {
                    // wide: the channel's own (unused) window serves kNJ trials at a
                    // time, trial i's samples t0 + d .. + len at i * kTB (dword loads:
                    // t + d <= T - 1 + max_delay = n - 1)
#pragma unroll
                    for (int i = 0; i < kNJ; ++i)
                        for (int q = tid; q < len; q += kDdThreads) win[cb][i * kTB + q] = row[d[cb][j + i] + q];
                    __syncthreads();
                }
                dd_accum<kNJ>(&acc[j], win[cb], off, tid);
                if (!staged[cb]) __syncthreads();
            }
        }
        __syncthreads();      // the next pair of channels overwrites the windows
    }
#pragma unroll
    for (int j = 0; j < kND; ++j) {
        if (j < nd) {
            float *o = o0 + (int64_t)j * orow + t0 + tid;
#pragma unroll
            for (int k = 0; k < kDdS; ++k)
                if (tid + k * kDdThreads < len) o[k * kDdThreads] = acc[j][k];
        }
    }
}

// (the pointers are separate __restrict__ parameters: the table is then known
// not to alias `out`, and its wave-uniform loads become scalar loads)
template <bool VEC>
__global__ __launch_bounds__(kDdThreads) void k_dedisperse(const float *__restrict__ data,
                                                           const int32_t *__restrict__ tab, float *__restrict__ out,
                                                           DdArgs a) {
    __shared__ __align__(16) float win[kCB][kWin];
    const int tid = threadIdx.x;
    // Workgroup id -> (time tile, trial group), groups fastest, through the XCD
    // run map: the trial groups of one time tile then run on one XCD, side by
    // side, and its L2 fetches each row once for all of them.
    const uint2 id = xcd_run_pair((unsigned)a.ngroups);
    const int g = (int)id.y;
    const int64_t t0 = (int64_t)id.x * kTB;
    const int j0 = g * kND;
    const int nd = min(kND, a.ndm - j0);                       // trials of this group (>= 1)
    const int len = (int)min((int64_t)kTB, a.T - t0);          // times of this tile (>= 1)
    dd_tile<VEC>(win, data, tab, out + (int64_t)j0 * a.out_ld, a.out_ld, 0, a.nchan, a.nchan, j0, nd, t0, len, a.n,
                 a.ld, a.max_delay, tid);
}

// the banded sum's own arguments, beside DdArgs (whose ngroups counts the trial
// groups of all sources): nsrc sources are in use, each but the last owns
// per_src trials = gps groups, the last one the rest
struct DdBandArgs {
    int64_t src_stride;
    int32_t band, nbands, per_src, nsrc, gps;
};

template <bool VEC>
__global__ __launch_bounds__(kDdThreads) void k_dedisperse_banded(const float *__restrict__ data,
                                                                  const int32_t *__restrict__ tab,
                                                                  float *__restrict__ out, DdArgs a, DdBandArgs b) {
    __shared__ __align__(16) float win[kCB][kWin];
    const int tid = threadIdx.x;
    // Workgroup id -> (time tile, band, trial group), groups fastest: the bands
    // and groups of one time tile run on one XCD and share its rows in that L2
    const uint2 id = xcd_run_pair((unsigned)a.ngroups);
    const int g = (int)id.y;
    const int s = (int)(id.x % (unsigned)b.nbands);
    const int64_t t0 = (int64_t)(id.x / (unsigned)b.nbands) * kTB;
    // the group's source, and its trials inside it: a group ends with its source
    const int q = min(g / b.gps, b.nsrc - 1);
    const int j0 = q * b.per_src + (g - q * b.gps) * kND;
    const int jend = q == b.nsrc - 1 ? a.ndm : (q + 1) * b.per_src;
    const int nd = min(kND, jend - j0);                        // (>= 1)
    const int len = (int)min((int64_t)kTB, a.T - t0);
    const int c_lo = s * b.band;
    const int c_hi = c_lo + min(b.band, a.nchan - c_lo);
    PSS_DASSERT(q >= 0 && j0 >= 0 && nd >= 1 && j0 + nd <= a.ndm && len >= 1 && c_lo < c_hi && c_hi <= a.nchan);
    dd_tile<VEC>(win, data + (int64_t)q * b.src_stride, tab, out + ((int64_t)j0 * b.nbands + s) * a.out_ld,
                 (int64_t)b.nbands * a.out_ld, c_lo, c_hi, a.nchan, j0, nd, t0, len, a.n, a.ld, a.max_delay, tid);
}

extern "C" {

int pss_dedisperse(const float *data, int32_t nchan, int64_t n, int64_t ld, const int32_t *delays, int32_t ndm,
                   int32_t max_delay, float *out, int64_t out_ld, void *stream) {
    if (!data) return fail(PSS_EINVAL, "dedisperse: data is NULL");
    if (!delays) return fail(PSS_EINVAL, "dedisperse: delays is NULL");
    if (!out) return fail(PSS_EINVAL, "dedisperse: out is NULL");
    if (nchan < 1) return fail(PSS_EINVAL, "dedisperse: nchan %d < 1", nchan);
    if (ndm < 1) return fail(PSS_EINVAL, "dedisperse: ndm %d < 1", ndm);
    if (ld < n) return fail(PSS_EINVAL, "dedisperse: ld %lld < n %lld", (long long)ld, (long long)n);
    if (max_delay < 0) return fail(PSS_EINVAL, "dedisperse: max_delay %d < 0", max_delay);
    if (max_delay >= n) return fail(PSS_EINVAL, "dedisperse: max_delay %d >= n %lld", max_delay, (long long)n);
    const int64_t T = n - max_delay;
    if (out_ld < T) return fail(PSS_EINVAL, "dedisperse: out_ld %lld < %lld output samples", (long long)out_ld,
                                (long long)T);
    const int64_t ngroups = ((int64_t)ndm + kND - 1) / kND;
    const int64_t ntiles = (T + kTB - 1) / kTB;
    const dim3 grid = grid_1d("dedisperse", ntiles, "time tiles", ngroups, "trial groups");
    if (!grid.x) return PSS_EINVAL;
    DdArgs a;
    a.n = n; a.ld = ld; a.nchan = nchan; a.ndm = ndm; a.max_delay = max_delay;
    a.ngroups = (int32_t)ngroups; a.out_ld = out_ld; a.T = T;
    // 16-B loads of the staged windows need the rows on the 16-B grid.  Same bits.
    if (on_grid16(data, ld))
        k_dedisperse<true><<<grid, dim3(kDdThreads), 0, (hipStream_t)stream>>>(data, delays, out, a);
    else
        k_dedisperse<false><<<grid, dim3(kDdThreads), 0, (hipStream_t)stream>>>(data, delays, out, a);
    LAUNCHCHK();
    return PSS_OK;
}

int pss_dedisperse_banded(const float *data, int32_t nsrc, int64_t src_stride, int32_t nchan, int64_t n, int64_t ld,
                          const int32_t *delays, int32_t ndm, int32_t per_src, int32_t max_delay, int32_t band,
                          float *out, int64_t out_ld, void *stream) {
    if (!data) return fail(PSS_EINVAL, "dedisperse_banded: data is NULL");
    if (!delays) return fail(PSS_EINVAL, "dedisperse_banded: delays is NULL");
    if (!out) return fail(PSS_EINVAL, "dedisperse_banded: out is NULL");
    if (nsrc < 1) return fail(PSS_EINVAL, "dedisperse_banded: nsrc %d < 1", nsrc);
    if (nchan < 1) return fail(PSS_EINVAL, "dedisperse_banded: nchan %d < 1", nchan);
    if (ndm < 1) return fail(PSS_EINVAL, "dedisperse_banded: ndm %d < 1", ndm);
    if (per_src < 1) return fail(PSS_EINVAL, "dedisperse_banded: per_src %d < 1", per_src);
    if (band < 1) return fail(PSS_EINVAL, "dedisperse_banded: band %d < 1", band);
    if (ld < n) return fail(PSS_EINVAL, "dedisperse_banded: ld %lld < n %lld", (long long)ld, (long long)n);
    if ((__int128)src_stride < (__int128)nchan * ld)
        return fail(PSS_EINVAL, "dedisperse_banded: src_stride %lld < nchan %d x ld %lld", (long long)src_stride, nchan,
                    (long long)ld);
    if (max_delay < 0) return fail(PSS_EINVAL, "dedisperse_banded: max_delay %d < 0", max_delay);
    if (max_delay >= n)
        return fail(PSS_EINVAL, "dedisperse_banded: max_delay %d >= n %lld", max_delay, (long long)n);
    const int64_t T = n - max_delay;
    if (out_ld < T) return fail(PSS_EINVAL, "dedisperse_banded: out_ld %lld < %lld output samples", (long long)out_ld,
                                (long long)T);
    // the sources in use; all but the last own per_src trials = gps groups
    const int64_t nsu = std::min<int64_t>(nsrc, ((int64_t)ndm + per_src - 1) / per_src);
    const int64_t last = ndm - (nsu - 1) * per_src;
    const int64_t gps = nsu > 1 ? ((int64_t)per_src + kND - 1) / kND : (last + kND - 1) / kND;
    const int64_t ngroups = (nsu - 1) * gps + (last + kND - 1) / kND;        // <= ndm
    const int64_t nbands = ((int64_t)nchan + band - 1) / band;
    const int64_t ntiles = (T + kTB - 1) / kTB;
    if (ntiles > (int64_t)0x7fffffff / nbands)
        return fail(PSS_EINVAL, "dedisperse_banded: %lld time tiles x %lld bands exceed 2^31 - 1 workgroups",
                    (long long)ntiles, (long long)nbands);
    const dim3 grid = grid_1d("dedisperse_banded", ntiles * nbands, "time tiles x bands", ngroups, "trial groups");
    if (!grid.x) return PSS_EINVAL;
    DdArgs a;
    a.n = n; a.ld = ld; a.nchan = nchan; a.ndm = ndm; a.max_delay = max_delay;
    a.ngroups = (int32_t)ngroups; a.out_ld = out_ld; a.T = T;
    DdBandArgs b;
    b.src_stride = src_stride; b.band = band; b.nbands = (int32_t)nbands; b.per_src = per_src;
    b.nsrc = (int32_t)nsu; b.gps = (int32_t)gps;
    // 16-B loads of the staged windows need every source's rows on the 16-B grid.  Same bits.
    if (on_grid16(data, ld) && (nsu == 1 || src_stride % 4 == 0))
        k_dedisperse_banded<true><<<grid, dim3(kDdThreads), 0, (hipStream_t)stream>>>(data, delays, out, a, b);
    else
        k_dedisperse_banded<false><<<grid, dim3(kDdThreads), 0, (hipStream_t)stream>>>(data, delays, out, a, b);
    LAUNCHCHK();
    return PSS_OK;
}

}  // extern "C"
