// pss_foldseries.hip -- fold of dedispersed series at fractional periods
// (extension, no reference counterpart): every output row folds one series of
// x at its own period and start phase into nsub sub-integrations of nbin phase
// bins.  The definition (include/pss_hip.h: pss_fold_series), wrapping uint64:
//
//   phi(u) = phi0 + u inc                        u = 0, 1, 2 .. sample of the series
//   bin(u) = ((phi(u) >> 32) nbin) >> 32
//   out [r][s][b] = float32(sum of x[i(r)][u], s L <= u < (s + 1) L, bin(u) = b)     (float64 sum)
//   hits[r][s][b] = number of such u
//
// In phases, bin b is the interval [E_b, E_b + W_b), E_b = ceil(b 2^32 / nbin)
// 2^32 -- bin(u) = b iff (phi(u) - E_b) mod 2^64 < W_b.  The samples of one bin
// in one turn are a contiguous run, and exactly one sample of a turn has an
// offset o = (phi(u) - E_b) mod 2^64 in [0, inc): the turn's "start" (its run is
// empty when o >= W_b, which only a period within 2^-32 of nbin samples can
// give).  With 2^64 = n inc + r, r < inc, the start after a start at (u, o) is
// (u + n, o - r) if o >= r and (u + n + 1, o - r + inc) otherwise: integer adds
// and compares, no division and no rounding -- the bins are exact.
//
//   k_fold_series<NS> : a workgroup of 256 threads owns one (row, sub-integration)
//       pair -- logical id = row nsub + sub through the XCD run map -- and
//       streams its L samples through LDS in chunks of kFsChunk, laid out from
//       the sub-integration's first sample whatever the address of that sample
//       is: a chunk's head up to the 16-B grid and its tail are element loads,
//       the body 16-B loads, all issued before the first LDS store; the same
//       values land in the same LDS words either way.  (LDS word e sits at
//       e + e / 32: runs of 32 k samples would put every lane on one bank.)
//       A thread owns bins and walks their runs out of LDS, adding in float64
//       in the order of u:
//         * nbin >= 256: thread t owns the bins t + 256 m, m < NS (NS = 1, 2, 4);
//         * nbin <  256: G = 256 / nbin threads share a bin (G > 1 for nbin <= 128), thread
//           t = g nbin + b is thread g of bin b.  Up to a period of CH / G samples
//           (floor(2^64 / inc) <= CH / G) it owns the turns g, g + G, g + 2 G .. counted
//           from the sub-integration's first start (its G-turn step (n_G, r_G) is G
//           steps of (n, r) added up); a run that is under way at the sub-integration's
//           first sample goes to g = 0.  A longer period has fewer than G turns in a
//           chunk, and the G threads split every run instead: with q = ceil((1 +
//           floor(Wmax / inc)) / G), Wmax the widest bin, thread g adds the samples
//           g q <= i < (g + 1) q of every run, i counted from the run's start (for the
//           run under way at the first sample: from its start before it) -- a counted
//           loop, the run's length is floor(W_b / inc) + (o < W_b mod inc).  (Periods
//           of 2^40 samples and more go turn by turn again: positions stay in 64 bits.)
//           At the end the G partial sums and counts of a bin go through LDS and
//           thread b adds them in the order g = 0 .. G - 1, rounds once and stores.
//       Which way a row goes, and the order of the adds, is a function of (L, nbin,
//       inc, phi0 + s L inc) alone: the bits depend on neither the run, the alignment of x / ld / out,
//       the position of the row nor the other rows.  No atomics, no workspace.
//       Sample positions are int64 relative to the sub-integration and saturate
//       at 2^62 (beyond any series that fits an address space); a cursor reads
//       LDS only at c0 <= u < c0 + n of the chunk that is staged.
#include "pss_common.hpp"

using namespace pss;

static constexpr int kFsThreads = 256;
static constexpr int kFsChunk = 4096;                     // samples staged per pass
static constexpr int kFsMaxBin = 1024;
static constexpr int kFsLds = kFsChunk + kFsChunk / 32;   // padded words
static constexpr uint64_t kFsFar = (uint64_t)1 << 62;     // "never": past every series
static constexpr uint64_t kFsSplitMax = (uint64_t)1 << 40;  // runs are split below this period (samples)

struct FoldArgs {
    int64_t T, ld, L;
    uint64_t inc_max;                                     // floor(2^64 / nbin)
    int32_t nser, nrows, nsub, nbin;
};

__device__ __forceinline__ int fs_pad(int e) { return e + (e >> 5); }

// E_b = ceil(b 2^32 / nbin) 2^32 (b = nbin: 2^64 = 0 mod 2^64)
__device__ __forceinline__ uint64_t fs_edge(uint32_t b, uint32_t nbin) {
    return ((((uint64_t)b << 32) + nbin - 1) / nbin) << 32;
}

// the start after the start (u, off): n samples on (one more when off < r)
__device__ __forceinline__ void fs_step(uint64_t &u, uint64_t &off, uint64_t n, uint64_t r, uint64_t inc) {
    const bool more = off < r;
    u = min(u + n + (more ? 1u : 0u), kFsFar);
    off = off - r + (more ? inc : 0);
}

// n valid samples of the chunk at p -> w (padded)
__device__ __forceinline__ void fs_stage(float *w, const float *p, int n, int tid) {
    constexpr int NP = kFsChunk / 4 / kFsThreads;         // 16-B loads per thread
    PSS_DASSERT(n >= 1 && n <= kFsChunk);
    const int head = min(n, (int)((4 - (((uintptr_t)p >> 2) & 3)) & 3));
    const int nb = (n - head) >> 2;                       // whole 16-B groups
    const int tail0 = head + 4 * nb;
    const float4 *body = reinterpret_cast<const float4 *>(p + head);
    float4 v[NP];
    float eh = 0.0f, et = 0.0f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int q = tid + i * kFsThreads;
        v[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (q < nb) v[i] = body[q];
    }
    if (tid < head) eh = p[tid];
    if (tail0 + tid < n) et = p[tail0 + tid];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const int q = tid + i * kFsThreads;
        if (q < nb) {
            const int e = head + 4 * q;
            PSS_DASSERT(e >= 0 && e + 3 < n);
            w[fs_pad(e)] = v[i].x;
            w[fs_pad(e + 1)] = v[i].y;
            w[fs_pad(e + 2)] = v[i].z;
            w[fs_pad(e + 3)] = v[i].w;
        }
    }
    if (tid < head) w[fs_pad(tid)] = eh;
    if (tail0 + tid < n) w[fs_pad(tail0 + tid)] = et;
}

// Turn by turn (short periods, and every row of nbin > 128): thread (b, g) walks the runs of the
// turns g, g + G, .. of bin b sample by sample; NS bins per thread when nbin > 256 (G = 1).
template <int NS>
__device__ __forceinline__ void fs_walk_turns(float *w, const float *row, const FoldArgs &a, int s, int tid,
                                              uint32_t nbin, int G, uint64_t inc, uint64_t p0, uint64_t n0,
                                              uint64_t r0, double (&acc)[NS], int (&cnt)[NS]) {
    // G turns on: G 2^64 = nG inc + rG, G steps of (n0, r0) added up
    uint64_t nG = 0, rG = 0;
    for (int i = 0; i < G; ++i) {
        rG += r0;
        const bool c = rG >= inc && inc != 0;
        if (c) rG -= inc;
        nG = min(nG + n0 + (c ? 1u : 0u), kFsFar);
    }
    uint64_t uc[NS], offc[NS], us[NS], off[NS], W[NS];
#pragma unroll
    for (int m = 0; m < NS; ++m) {
        const uint32_t b = NS == 1 ? (uint32_t)tid % nbin : (uint32_t)(tid + m * kFsThreads);
        const int g = NS == 1 ? tid / (int)nbin : 0;
        const bool active = NS == 1 ? g < G : b < nbin;
        acc[m] = 0.0;
        cnt[m] = 0;
        const uint64_t E = fs_edge(active ? b : 0, nbin);
        W[m] = fs_edge((active ? b : 0) + 1, nbin) - E;
        const uint64_t o0 = p0 - E;                        // offset of the first sample
        // the first start at or after the first sample
        uint64_t u1 = 0, o1 = o0;
        if (o0 >= inc) {
            if (inc != 0) {
                const uint64_t xx = 0 - o0;                // 1 .. 2^64 - inc
                const uint64_t d = (xx + inc - 1) / inc;
                o1 = d * inc - xx;
                u1 = min(d, kFsFar);
            } else {
                u1 = kFsFar;
            }
        }
        for (int i = 0; i < g; ++i) fs_step(u1, o1, n0, r0, inc);
        us[m] = active ? u1 : kFsFar;
        off[m] = o1;
        // the cursor: a run under way at the first sample (g = 0), else "jump to the next start"
        uc[m] = active ? 0 : kFsFar;
        offc[m] = (g == 0 && o0 >= inc) ? o0 : ~(uint64_t)0;
    }
    for (int64_t c0 = 0; c0 < a.L; c0 += kFsChunk) {
        const int n = (int)min((int64_t)kFsChunk, a.L - c0);
        if (c0 > 0) __syncthreads();                       // the previous chunk's reads are done
        PSS_DASSERT((int64_t)s * a.L + c0 + n <= a.T);
        fs_stage(w, row + c0, n, tid);
        __syncthreads();
        const uint64_t c1 = (uint64_t)c0 + (uint64_t)n;
#pragma unroll
        for (int m = 0; m < NS; ++m) {
            for (;;) {
                if (uc[m] >= c1) break;
                if (offc[m] >= W[m]) {                     // outside the bin: on to this thread's next start
                    uc[m] = us[m];
                    offc[m] = off[m];
                    fs_step(us[m], off[m], nG, rG, inc);
                    continue;
                }
                const int e = (int)(uc[m] - (uint64_t)c0);
                PSS_DASSERT(uc[m] >= (uint64_t)c0 && e >= 0 && e < n);
                acc[m] += (double)w[fs_pad(e)];
                ++cnt[m];
                ++uc[m];
                offc[m] += inc;
            }
        }
    }
}

// Run by run (nbin <= 128 and a period of more than CH / G samples, below 2^40): every thread
// walks every turn of its bin, and of a run of len samples thread (b, g) adds the samples
// g q <= i < min((g + 1) q, len) counted from the run's start -- a counted loop, no phase per
// sample: with W_b = Rb inc + wb a run from a start at offset o has len = Rb + (o < wb).
__device__ __forceinline__ void fs_walk_runs(float *w, const float *row, const FoldArgs &a, int s, int tid,
                                             uint32_t nbin, int G, uint64_t inc, uint64_t p0, uint64_t n0,
                                             uint64_t r0, double &acc, int &cnt) {
    const uint32_t b = (uint32_t)tid % nbin;
    const int g = tid / (int)nbin;
    const bool active = g < G;
    const uint64_t E = fs_edge(b, nbin);
    const uint64_t Wb = fs_edge(b + 1, nbin) - E;
    const uint64_t Rb = Wb / inc, wb = Wb - Rb * inc;
    // the part of a thread: q samples, G q >= 1 + the longest Rb of any bin
    const uint64_t Wmax = ((((uint64_t)1 << 32) + nbin - 1) / nbin) << 32;
    const int64_t q = (int64_t)((Wmax / inc + (uint64_t)G) / (uint64_t)G);
    // the start at or before the first sample, i0 samples back (i0 <= n0 < 2^40)
    const uint64_t o0 = p0 - E;
    const uint64_t i0 = o0 / inc;
    uint64_t ov = o0 - i0 * inc;
    int64_t uv = active ? -(int64_t)i0 : (int64_t)kFsFar;
    int64_t pc = 0, pe = 0;                                // the part under way: [pc, pe)
    double sum = 0.0;
    int num = 0;
    for (int64_t c0 = 0; c0 < a.L; c0 += kFsChunk) {
        const int n = (int)min((int64_t)kFsChunk, a.L - c0);
        if (c0 > 0) __syncthreads();                       // the previous chunk's reads are done
        PSS_DASSERT((int64_t)s * a.L + c0 + n <= a.T);
        fs_stage(w, row + c0, n, tid);
        __syncthreads();
        const int64_t c1 = c0 + n;
        for (;;) {
            if (pc >= pe) {                                // part done: this thread's part of the next run
                if (uv >= c1) break;
                const int64_t len = (int64_t)Rb + (ov < wb ? 1 : 0);
                PSS_DASSERT(len <= (int64_t)G * q);
                pc = max(uv + (int64_t)g * q, (int64_t)0);
                pe = uv + min((int64_t)(g + 1) * q, len);
                const bool more = ov < r0;
                uv += (int64_t)n0 + (more ? 1 : 0);
                ov = ov - r0 + (more ? inc : 0);
                continue;
            }
            if (pc >= c1) break;
            const int e0 = (int)(pc - c0), e1 = (int)(min(pe, c1) - c0);
            PSS_DASSERT(e0 >= 0 && e0 < e1 && e1 <= n);
            for (int e = e0; e < e1; ++e) sum += (double)w[fs_pad(e)];
            num += e1 - e0;
            pc = c0 + e1;
        }
    }
    acc = sum;
    cnt = num;
}

template <int NS>
__global__ __launch_bounds__(kFsThreads) void k_fold_series(const float *__restrict__ x,
                                                            const int32_t *__restrict__ src,
                                                            const uint64_t *__restrict__ inc_t,
                                                            const uint64_t *__restrict__ phi0_t,
                                                            float *__restrict__ out, int32_t *__restrict__ hits,
                                                            FoldArgs a) {
    __shared__ __align__(16) float w[kFsLds];
    static_assert(kFsLds * 4 >= kFsThreads * 12, "the partial sums and counts fit the staging buffer");
    const int tid = threadIdx.x;
    const uint32_t nbin = (uint32_t)a.nbin;
    PSS_DASSERT(nbin >= 2 && nbin <= (uint32_t)(NS * kFsThreads) && (NS == 1 || nbin > (uint32_t)(NS / 2 * kFsThreads)));

    // workgroup id -> (row, sub-integration), sub-integrations fastest, through the XCD run map
    const uint2 id = xcd_run_pair((unsigned)a.nsub);
    const int r = (int)id.x;
    const int s = (int)id.y;
    PSS_DASSERT(r >= 0 && r < a.nrows);
    const int ser = min(max(src[r], 0), a.nser - 1);
    const uint64_t inc = min(inc_t[r], a.inc_max);
    const uint64_t p0 = (phi0_t ? phi0_t[r] : 0) + (uint64_t)((int64_t)s * a.L) * inc;   // phi(s L)
    const float *row = x + (int64_t)ser * a.ld + (int64_t)s * a.L;

    // 2^64 = n0 inc + r0 (inc = 0: every sample has the phase p0 and no turn ever starts)
    uint64_t n0 = kFsFar, r0 = 0;
    if (inc != 0) {
        const uint64_t q = ~(uint64_t)0 / inc, rem = ~(uint64_t)0 % inc;   // 2^64 - 1 = q inc + rem
        const bool carry = rem + 1 == inc;
        r0 = carry ? 0 : rem + 1;
        n0 = q >= kFsFar ? kFsFar : q + (carry ? 1u : 0u);
    }
    // who shares a bin: G threads, thread tid = g nbin + b takes every G-th turn
    const int G = NS == 1 ? max(1, kFsThreads / (int)nbin) : 1;

    double acc[NS];
    int cnt[NS];
    // A turn longer than CH / G samples puts fewer than G turns into a chunk and would leave the
    // threads of the other turns idle: the G threads of a bin then split every run instead.
    // (Uniform in the workgroup: a property of the row.)
    if (NS == 1 && G > 1 && n0 > (uint64_t)(kFsChunk / G) && n0 < kFsSplitMax)
        fs_walk_runs(w, row, a, s, tid, nbin, G, inc, p0, n0, r0, acc[0], cnt[0]);
    else
        fs_walk_turns<NS>(w, row, a, s, tid, nbin, G, inc, p0, n0, r0, acc, cnt);

    const int64_t obase = ((int64_t)r * a.nsub + s) * (int64_t)nbin;
    if (NS == 1 && G > 1) {
        // the G partials of a bin, added in the order g = 0 .. G - 1 by thread b
        __syncthreads();
        double *pd = reinterpret_cast<double *>(w);
        int *pc = reinterpret_cast<int *>(pd + kFsThreads);
        if (tid < G * (int)nbin) {
            pd[tid] = acc[0];
            pc[tid] = cnt[0];
        }
        __syncthreads();
        if (tid < (int)nbin) {
            double sum = pd[tid];
            int c = pc[tid];
            for (int g = 1; g < G; ++g) {
                PSS_DASSERT(g * (int)nbin + tid < kFsThreads);
                sum += pd[g * (int)nbin + tid];
                c += pc[g * (int)nbin + tid];
            }
            out[obase + tid] = (float)sum;
            if (hits) hits[obase + tid] = c;
        }
        return;
    }
#pragma unroll
    for (int m = 0; m < NS; ++m) {
        const int b = tid + m * kFsThreads;
        if (b < (int)nbin) {
            out[obase + b] = (float)acc[m];
            if (hits) hits[obase + b] = cnt[m];
        }
    }
}

extern "C" {

int pss_fold_series(const float *x, int32_t nser, int64_t T, int64_t ld, const int32_t *src, const uint64_t *inc,
                    const uint64_t *phi0, int32_t nrows, int32_t nsub, int64_t L, int32_t nbin, float *out,
                    int32_t *hits, void *stream) {
    if (!x) return fail(PSS_EINVAL, "fold_series: x is NULL");
    if (!src) return fail(PSS_EINVAL, "fold_series: src is NULL");
    if (!inc) return fail(PSS_EINVAL, "fold_series: inc is NULL");
    if (!out) return fail(PSS_EINVAL, "fold_series: out is NULL");
    if (nser < 1) return fail(PSS_EINVAL, "fold_series: nser %d < 1", nser);
    if (nrows < 1) return fail(PSS_EINVAL, "fold_series: nrows %d < 1", nrows);
    if (nsub < 1) return fail(PSS_EINVAL, "fold_series: nsub %d < 1", nsub);
    if (L < 1) return fail(PSS_EINVAL, "fold_series: L %lld < 1", (long long)L);
    if (T < 1 || L > T / nsub)
        return fail(PSS_EINVAL, "fold_series: nsub %d x L %lld > T %lld", nsub, (long long)L, (long long)T);
    if (ld < T) return fail(PSS_EINVAL, "fold_series: ld %lld < T %lld", (long long)ld, (long long)T);
    if (nbin < 2 || nbin > kFsMaxBin) return fail(PSS_EINVAL, "fold_series: nbin %d outside [2, %d]", nbin, kFsMaxBin);
    const dim3 grid = grid_1d("fold_series", nrows, "rows", nsub, "sub-integrations");
    if (!grid.x) return PSS_EINVAL;
    FoldArgs a;
    a.T = T; a.ld = ld; a.L = L;
    a.nser = nser; a.nrows = nrows; a.nsub = nsub; a.nbin = nbin;
    // floor(2^64 / nbin) from 2^64 - 1 = q nbin + rem
    a.inc_max = ~(uint64_t)0 / (uint64_t)nbin + (~(uint64_t)0 % (uint64_t)nbin == (uint64_t)nbin - 1 ? 1 : 0);
    hipStream_t st = (hipStream_t)stream;
    if (nbin <= kFsThreads)
        k_fold_series<1><<<grid, dim3(kFsThreads), 0, st>>>(x, src, inc, phi0, out, hits, a);
    else if (nbin <= 2 * kFsThreads)
        k_fold_series<2><<<grid, dim3(kFsThreads), 0, st>>>(x, src, inc, phi0, out, hits, a);
    else
        k_fold_series<4><<<grid, dim3(kFsThreads), 0, st>>>(x, src, inc, phi0, out, hits, a);
    LAUNCHCHK();
    return PSS_OK;
}

}  // extern "C"
