// pss_ffa.hip -- fast folding search of the DM-time plane (extension, no
// reference counterpart): the time scrunch of a trial by 2^lf, the fast folding
// transform of the scrunched series at every base period of a call, and the
// circular boxcar search of its profiles.  The definitions (include/pss_hip.h:
// pss_ffa_scrunch, pss_ffa_transform, pss_ffa_profile_search) are all in IEEE
// float32, one rounded operation per line; every index is an integer.
//
// The transform of one (series, base period p) block of m = n / p rows of p
// samples is the top-down halving tree
//     F(a, 1) = row a,   F(a, m) = combine(F(a, h), F(a + h, m - h)),  h = m / 2,
//     F_s[f] = H_{i_s}[f] + Tl_{j_s}[(f + b_s) mod p]
// whose node (a, m) lives in rows a .. a + m - 1 of the block, at every level.
// A level is computed from the level below it out of place, so the levels
// ping-pong between `out` and `work`: depth d is written to `out` when d is
// even, and the root (d = 0) therefore ends in `out`.
//
//   k_ffa_level : one global level, depth d from depth d + 1.  A wave owns one
//       output row at a time (four rows a workgroup): it descends the tree
//       from the root to the row's node -- at most 27 uniform integer steps --
//       forms (i_s, j_s, b_s), and adds the two source rows, lane f on sample
//       f, f + 64 ..: consecutive lanes on consecutive dwords of H, of the
//       output and of each of the two contiguous runs of the rotated row (the
//       rotation is an add and one conditional subtract, no division and no
//       gather).  A node of one row is a copy.
//   k_ffa_fused : the bottom of the tree.  The subtree under a node of depth
//       dF, the smallest depth whose nodes hold at most kFfaLds floats, is
//       computed by one workgroup: its leaves are read from y once, its levels
//       ping-pong between two LDS buffers and its root level is written once.
//       The log2 of its rows levels cost one pass over the block instead of
//       one each.  The tree is the same, so the bits are those of k_ffa_level
//       run from the leaves (built with -DPSS_FFA_NO_FUSE=1 the library takes
//       that route for every level: the A/B of tools/ffa_bench.py).
//   k_ffa_search : a workgroup owns one cell of `cell` profiles of one block.
//       A profile of up to 1024 bins is searched by one wave (four profiles at
//       a time), a longer one by the whole workgroup: the row is staged in LDS,
//       level k + 1 is written next to level k (S + its circular partner 2^k
//       bins on), every thread keeps the best (z, key) of what it has seen
//       under cm_better (pss_cellmax.hpp), key = k << 23 | (s - q cell) << 12 |
//       f, and the 256 are reduced by wave shuffles and four LDS words.  (The
//       per-cell butterfly of cm_reduce_store assumes one entry per tile slot
//       and a two-word result: it is left as the two time / bin searches use
//       it.)
//   k_ffa_scrunch : a thread owns one output sample and sums its 2^lf inputs
//       in the pairwise tree with a binary counter of partial sums in
//       registers.
// No atomics, no allocation, no table from the caller.
#include "pss_cellmax.hpp"

using namespace pss;

static constexpr int kFfaThreads = 256;
static constexpr int kFfaWaves = kFfaThreads / 64;
#ifndef PSS_FFA_FUSED_THREADS
#define PSS_FFA_FUSED_THREADS 512                        // (the A/B of tools/ffa_bench.py builds 256 and 1024)
#endif
static constexpr int kFfaFusedThreads = PSS_FFA_FUSED_THREADS;   // the LDS subtrees: 64 KB a workgroup, two a CU
static constexpr int kFfaFusedWaves = kFfaFusedThreads / 64;
static constexpr int kFfaLds = 8192;                      // floats of one LDS level buffer (two rows of the longest period)
static constexpr int kFfaMaxP = 4096;                     // longest base period
static constexpr int kFfaMaxLf = 16;
static constexpr int kFfaMaxW = 11;                       // widths 2^0 .. 2^10
static constexpr int kFfaWaveP = 1024;                    // profiles up to here are searched by one wave

struct FfaArgs {
    int64_t n, ld;
    int32_t nser, p0, np, d;
    uint32_t per_block;                                   // workgroups per (series, period) block
};

struct FfaSearchArgs {
    int64_t n, out_ld;
    int32_t nser, p0, np, nw, cell, lcell;
    uint32_t nq;
};

// ceil(log2 m): the depth of the tree of m rows
__host__ __device__ static inline int ffa_depth(int m) {
    int d = 0;
    while ((1 << d) < m) ++d;
    return d;
}

// the smallest depth whose nodes (at most ceil(m / 2^d) rows each) fit one LDS buffer
__host__ __device__ static inline int ffa_fuse_depth(int m, int p) {
    int d = 0;
    while ((int64_t)((m + (1 << d) - 1) >> d) * p > kFfaLds) ++d;
    return d;
}

// the node (a, m) of `depth` levels below the node (a, m) given that holds row r
__device__ __forceinline__ void ffa_descend(int &a, int &m, int r, int depth) {
    for (int l = 0; l < depth && m > 1; ++l) {
        const int h = m >> 1;
        if (r < a + h) {
            m = h;
        } else {
            a += h;
            m -= h;
        }
    }
}

// (i_s, j_s, b_s) of output row s of a node of m >= 2 rows
__device__ __forceinline__ void ffa_rule(int m, int s, int &i, int &j, int &b) {
    const int h = m >> 1, t = m - h;
    if (m <= 32768) {                                      // 2 s h < 2^30
        const uint32_t den = 2u * (uint32_t)(m - 1), s2 = 2u * (uint32_t)s, rnd = (uint32_t)(m - 1);
        i = (int)((s2 * (uint32_t)(h - 1) + rnd) / den);
        j = (int)((s2 * (uint32_t)(t - 1) + rnd) / den);
        b = (int)((s2 * (uint32_t)h + rnd) / den);
    } else {
        const int64_t den = 2 * (int64_t)(m - 1), s2 = 2 * (int64_t)s, rnd = m - 1;
        i = (int)((s2 * (h - 1) + rnd) / den);
        j = (int)((s2 * (t - 1) + rnd) / den);
        b = (int)((s2 * h + rnd) / den);
    }
}

// dst[f] = H[f] + T[(f + b) mod p], f < p, by one wave; 0 <= b < p
__device__ __forceinline__ void ffa_row_add(float *dst, const float *H, const float *T, int p, int b, int lane) {
#pragma unroll 4
    for (int f = lane; f < p; f += 64) {
        int g = f + b;
        g -= g >= p ? p : 0;
        dst[f] = H[f] + T[g];
    }
}

__device__ __forceinline__ void ffa_row_copy(float *dst, const float *src, int p, int lane) {
#pragma unroll 4
    for (int f = lane; f < p; f += 64) dst[f] = src[f];
}

// One output row of depth `depth` below the node (a, m): row r of dst from the
// rows of src (both indexed by the row's number minus `base`).
__device__ __forceinline__ void ffa_row(float *dst, const float *src, int a, int m, int r, int depth, int base, int p,
                                        int lane) {
    ffa_descend(a, m, r, depth);
    PSS_DASSERT(r >= a && r < a + m);
    float *o = dst + (int64_t)(r - base) * p;
    if (m == 1) {
        ffa_row_copy(o, src + (int64_t)(r - base) * p, p, lane);
        return;
    }
    int i, j, b;
    ffa_rule(m, r - a, i, j, b);
    b %= p;                                                // (b_s <= m / 2 can pass p: one uniform division a row)
    PSS_DASSERT(i >= 0 && i < (m >> 1) && j >= 0 && j < m - (m >> 1) && b >= 0 && b < p);
    ffa_row_add(o, src + (int64_t)(a + i - base) * p, src + (int64_t)(a + (m >> 1) + j - base) * p, p, b, lane);
}

template <bool FUSED>
__global__ __launch_bounds__(kFfaThreads) void k_ffa_level(const float *__restrict__ y, float *out, float *work,
                                                           FfaArgs a) {
    const uint2 id = xcd_run_pair(a.per_block);
    const int blk = (int)id.x;
    const int i = blk / a.np, pi = blk - i * a.np, p = a.p0 + pi;
    const int m = (int)(a.n / p);
    // the block's levels are the depths below `top`
    const int top = FUSED ? ffa_fuse_depth(m, p) : max(ffa_depth(m), 1);
    if (a.d >= top) return;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int r = (int)id.y * kFfaWaves + wave;
    if (r >= m) return;
    PSS_DASSERT(i < a.nser && (int64_t)(r + 1) * p <= a.n);
    const int64_t off = (int64_t)blk * a.n;
    float *dst = ((a.d & 1) ? work : out) + off;
    const float *src = (!FUSED && a.d == top - 1) ? y + (int64_t)i * a.ld : ((a.d & 1) ? out : work) + off;
    ffa_row(dst, src, 0, m, r, a.d, 0, p, (int)(threadIdx.x & 63));
}

__global__ __launch_bounds__(kFfaFusedThreads) void k_ffa_fused(const float *__restrict__ y, float *out, float *work,
                                                           FfaArgs a) {
    __shared__ float lev[2][kFfaLds];
    const uint2 id = xcd_run_pair(a.per_block);
    const int blk = (int)id.x;
    const int i = blk / a.np, pi = blk - i * a.np, p = a.p0 + pi;
    const int m = (int)(a.n / p);
    const int dF = ffa_fuse_depth(m, p);
    const int node = (int)id.y;
    if (node >= (1 << dF)) return;                         // (uniform: this period has fewer subtrees)
    // node number `node` of depth dF: its bits, the highest first, are the turns from the root
    int a0 = 0, M = m;
    for (int l = 0; l < dF; ++l) {
        const int h = M >> 1;
        if ((node >> (dF - 1 - l)) & 1) {
            a0 += h;
            M -= h;
        } else {
            M = h;
        }
    }
    PSS_DASSERT(M >= 1 && (int64_t)M * p <= kFfaLds && (int64_t)(a0 + M) * p <= a.n);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane = (int)(threadIdx.x & 63);
    const float *leaves = y + (int64_t)i * a.ld + (int64_t)a0 * p;
    float *root = ((dF & 1) ? work : out) + (int64_t)blk * a.n + (int64_t)a0 * p;
    const int nst = max(ffa_depth(M), 1);                  // levels of the subtree
    int cur = 0;
    for (int st = nst - 1; st >= 0; --st) {
        const bool first = st == nst - 1, last = st == 0;
        for (int r = a0 + wave; r < a0 + M; r += kFfaFusedWaves) {
            if (first && last)
                ffa_row(root, leaves, a0, M, r, st, a0, p, lane);
            else if (first)
                ffa_row(lev[cur], leaves, a0, M, r, st, a0, p, lane);
            else if (last)
                ffa_row(root, lev[cur ^ 1], a0, M, r, st, a0, p, lane);
            else
                ffa_row(lev[cur], lev[cur ^ 1], a0, M, r, st, a0, p, lane);
        }
        if (!last) {
            __syncthreads();
            cur ^= 1;
        }
    }
}

__global__ __launch_bounds__(kFfaThreads) void k_ffa_search(const float *__restrict__ prof,
                                                            const float *__restrict__ rstd,
                                                            const float *__restrict__ rm, float *__restrict__ snr,
                                                            int32_t *__restrict__ code, int32_t *__restrict__ phase,
                                                            FfaSearchArgs a) {
    __shared__ float buf[2][kFfaMaxP];
    __shared__ float redz[kFfaWaves];
    __shared__ int redc[kFfaWaves];
    const int tid = threadIdx.x;
    const uint2 id = xcd_run_pair(a.nq);
    const int blk = (int)id.x, q = (int)id.y;
    const int i = blk / a.np, pi = blk - i * a.np, p = a.p0 + pi;
    const int m = (int)(a.n / p);
    const int nqp = (m + a.cell - 1) >> a.lcell;
    const int64_t o = (int64_t)blk * a.out_ld + q;
    if (q >= nqp) {                                        // (uniform) a cell this period does not have
        if (tid == 0) {
            snr[o] = -INFINITY;
            code[o] = 0;
            phase[o] = 0;
        }
        return;
    }
    const float g = rstd[i] * rm[pi];
    // a profile is searched by one wave (four at a time) or by the workgroup
    const bool wide = p > kFfaWaveP;
    const int G = wide ? kFfaThreads : 64, ng = wide ? 1 : kFfaWaves;
    const int grp = wide ? 0 : tid >> 6, gl = wide ? tid : tid & 63;
    const int region = wide ? 0 : grp * kFfaWaveP;
    int nlev = 0;
    while (nlev < a.nw && (2 << nlev) <= p) ++nlev;
    const int s0 = q << a.lcell, s1 = min(s0 + a.cell, m);
    const float *rows = prof + (int64_t)blk * a.n;
    float bz = -INFINITY;
    int bkey = 0x7fffffff;
    for (int sb = s0; sb < s1; sb += ng) {                 // (uniform trip count: the barriers are met by all)
        const int s = sb + grp;
        const bool active = s < s1;
        float *cur = buf[0] + region, *nxt = buf[1] + region;
        if (active) {
            PSS_DASSERT((int64_t)(s + 1) * p <= a.n);
            const float *row = rows + (int64_t)s * p;
            for (int f = gl; f < p; f += G) cur[f] = row[f];
        }
        __syncthreads();
        for (int k = 0; k < nlev; ++k) {
            const bool more = k + 1 < nlev;
            if (active) {
                const float ak = cm_coef(k);
                const int step = 1 << k;
                const int key0 = (k << 23) | ((s - s0) << 12);
                for (int f = gl; f < p; f += G) {
                    const float S = cur[f];
                    const float w = S * ak;
                    const float z = w * g;
                    if (cm_better(z, key0 | f, bz, bkey)) {
                        bz = z;
                        bkey = key0 | f;
                    }
                    if (more) {
                        int f2 = f + step;
                        f2 -= f2 >= p ? p : 0;
                        nxt[f] = S + cur[f2];
                    }
                }
            }
            if (more) {
                __syncthreads();
                float *t = cur;
                cur = nxt;
                nxt = t;
            }
        }
        __syncthreads();                                   // the next profile overwrites the buffers
    }
    for (int off = 1; off < 64; off <<= 1) {
        const float oz = __shfl_xor(bz, off);
        const int oc = __shfl_xor(bkey, off);
        if (cm_better(oz, oc, bz, bkey)) {
            bz = oz;
            bkey = oc;
        }
    }
    if ((tid & 63) == 0) {
        redz[tid >> 6] = bz;
        redc[tid >> 6] = bkey;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kFfaWaves; ++w)
            if (cm_better(redz[w], redc[w], bz, bkey)) {
                bz = redz[w];
                bkey = redc[w];
            }
        const bool none = bz == -INFINITY;
        PSS_DASSERT(q < a.out_ld);
        snr[o] = bz;
        code[o] = none ? 0 : ((bkey >> 23) << 16) | ((bkey >> 12) & 0x7ff);
        phase[o] = none ? 0 : bkey & 0xfff;
    }
}

template <bool SUB>
__global__ __launch_bounds__(kFfaThreads) void k_ffa_scrunch(const float *__restrict__ x,
                                                             const float *__restrict__ sub, float *__restrict__ y,
                                                             int64_t ld, int64_t y_ld, int64_t n, int lf,
                                                             uint32_t ntiles) {
    const uint2 id = xcd_run_pair(ntiles);
    const int i = (int)id.x;
    const int64_t u = (int64_t)id.y * kFfaThreads + threadIdx.x;
    if (u >= n) return;
    const float *px = x + (int64_t)i * ld + (u << lf);
    const float mu = SUB ? sub[i] : 0.0f;
    const int count = 1 << lf;
    float st[kFfaMaxLf + 1];                               // st[b]: the left sibling waiting at level b
    float v = 0.0f;
    for (int c = 0; c < count; ++c) {
        v = px[c];
        if (SUB) v = v - mu;
#pragma unroll
        for (int b = 0; b <= kFfaMaxLf; ++b) {
            if (!((c >> b) & 1)) {
                st[b] = v;
                break;
            }
            v = st[b] + v;
        }
    }
    y[(int64_t)i * y_ld + u] = v;                          // (the last sample closed every level up to lf)
}

// the checks the transform and the profile search share; m = n / p >= 1 for every period
static int ffa_check(const char *what, int32_t nser, int64_t n, int32_t p0, int32_t np) {
    if (nser < 1) return fail(PSS_EINVAL, "%s: nser %d < 1", what, nser);
    if (p0 < 2) return fail(PSS_EINVAL, "%s: p0 %d < 2", what, p0);
    if (np < 1) return fail(PSS_EINVAL, "%s: np %d < 1", what, np);
    if (n > ((int64_t)1 << 28)) return fail(PSS_EINVAL, "%s: n %lld > 2^28", what, (long long)n);
    const int64_t pmax = (int64_t)p0 + np - 1;
    if (pmax > n || pmax > kFfaMaxP)
        return fail(PSS_EINVAL, "%s: the longest period %lld exceeds min(n %lld, %d)", what, (long long)pmax,
                    (long long)n, kFfaMaxP);
    return PSS_OK;
}

extern "C" {

int pss_ffa_scrunch(const float *x, int32_t nser, int64_t T, int64_t ld, const float *sub, int32_t lf, float *y,
                    int64_t y_ld, void *stream) {
    if (!x) return fail(PSS_EINVAL, "ffa_scrunch: x is NULL");
    if (!y) return fail(PSS_EINVAL, "ffa_scrunch: y is NULL");
    if (nser < 1) return fail(PSS_EINVAL, "ffa_scrunch: nser %d < 1", nser);
    if (lf < 0 || lf > kFfaMaxLf) return fail(PSS_EINVAL, "ffa_scrunch: lf %d outside [0, %d]", lf, kFfaMaxLf);
    if (T < 1 || (T >> lf) < 1)
        return fail(PSS_EINVAL, "ffa_scrunch: T %lld holds no sample of 2^%d", (long long)T, lf);
    if (ld < T) return fail(PSS_EINVAL, "ffa_scrunch: ld %lld < T %lld", (long long)ld, (long long)T);
    const int64_t n = T >> lf;
    if (y_ld < n) return fail(PSS_EINVAL, "ffa_scrunch: y_ld %lld < %lld samples", (long long)y_ld, (long long)n);
    const int64_t ntiles = (n - 1) / kFfaThreads + 1;
    const dim3 grid = grid_1d("ffa_scrunch", ntiles, "tiles", nser, "series");
    if (!grid.x) return PSS_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (sub)
        k_ffa_scrunch<true><<<grid, dim3(kFfaThreads), 0, st>>>(x, sub, y, ld, y_ld, n, lf, (uint32_t)ntiles);
    else
        k_ffa_scrunch<false><<<grid, dim3(kFfaThreads), 0, st>>>(x, sub, y, ld, y_ld, n, lf, (uint32_t)ntiles);
    LAUNCHCHK();
    return PSS_OK;
}

int pss_ffa_transform(const float *y, int32_t nser, int64_t n, int64_t ld, int32_t p0, int32_t np, float *out,
                      float *work, void *stream) {
    if (!y) return fail(PSS_EINVAL, "ffa_transform: y is NULL");
    if (!out) return fail(PSS_EINVAL, "ffa_transform: out is NULL");
    if (!work) return fail(PSS_EINVAL, "ffa_transform: work is NULL");
    if (ffa_check("ffa_transform", nser, n, p0, np)) return PSS_EINVAL;
    if (ld < n) return fail(PSS_EINVAL, "ffa_transform: ld %lld < n %lld", (long long)ld, (long long)n);
    const int64_t blocks = (int64_t)nser * np;
    const int mmax = (int)(n / p0);
    int dfmax = 0;
    for (int pi = 0; pi < np; ++pi) dfmax = max(dfmax, ffa_fuse_depth((int)(n / (p0 + pi)), p0 + pi));
    const int64_t rowgroups = (mmax - 1) / kFfaWaves + 1;
    // both grids are checked whichever route is built: the rejections do not depend on it
    const dim3 glev = grid_1d("ffa_transform", rowgroups, "row groups", blocks, "blocks");
    if (!glev.x) return PSS_EINVAL;
    const dim3 gfus = grid_1d("ffa_transform", (int64_t)1 << dfmax, "subtrees", blocks, "blocks");
    if (!gfus.x) return PSS_EINVAL;
    FfaArgs a;
    a.n = n; a.ld = ld; a.nser = nser; a.p0 = p0; a.np = np; a.d = 0;
    hipStream_t st = (hipStream_t)stream;
#ifdef PSS_FFA_NO_FUSE
    a.per_block = (uint32_t)rowgroups;
    for (int d = max(ffa_depth(mmax), 1) - 1; d >= 0; --d) {
        a.d = d;
        k_ffa_level<false><<<glev, dim3(kFfaThreads), 0, st>>>(y, out, work, a);
        LAUNCHCHK();
    }
#else
    a.per_block = 1u << dfmax;
    k_ffa_fused<<<gfus, dim3(kFfaFusedThreads), 0, st>>>(y, out, work, a);
    LAUNCHCHK();
    a.per_block = (uint32_t)rowgroups;
    for (int d = dfmax - 1; d >= 0; --d) {
        a.d = d;
        k_ffa_level<true><<<glev, dim3(kFfaThreads), 0, st>>>(y, out, work, a);
        LAUNCHCHK();
    }
#endif
    return PSS_OK;
}

int pss_ffa_profile_search(const float *prof, int32_t nser, int64_t n, int32_t p0, int32_t np, const float *rstd,
                           const float *rm, int32_t nw, int32_t cell, float *snr, int32_t *code, int32_t *phase,
                           int64_t out_ld, void *stream) {
    if (!prof) return fail(PSS_EINVAL, "ffa_profile_search: prof is NULL");
    if (!rstd) return fail(PSS_EINVAL, "ffa_profile_search: rstd is NULL");
    if (!rm) return fail(PSS_EINVAL, "ffa_profile_search: rm is NULL");
    if (!snr) return fail(PSS_EINVAL, "ffa_profile_search: snr is NULL");
    if (!code) return fail(PSS_EINVAL, "ffa_profile_search: code is NULL");
    if (!phase) return fail(PSS_EINVAL, "ffa_profile_search: phase is NULL");
    if (ffa_check("ffa_profile_search", nser, n, p0, np)) return PSS_EINVAL;
    if (nw < 1 || nw > kFfaMaxW)
        return fail(PSS_EINVAL, "ffa_profile_search: nw %d outside [1, %d]", nw, kFfaMaxW);
    if (check_cell("ffa_profile_search", cell, 2048)) return PSS_EINVAL;
    const int64_t nq = (n / p0 - 1) / cell + 1;
    if (out_ld < nq)
        return fail(PSS_EINVAL, "ffa_profile_search: out_ld %lld < %lld cells", (long long)out_ld, (long long)nq);
    const dim3 grid = grid_1d("ffa_profile_search", nq, "cells", (int64_t)nser * np, "blocks");
    if (!grid.x) return PSS_EINVAL;
    FfaSearchArgs a;
    a.n = n; a.out_ld = out_ld; a.nser = nser; a.p0 = p0; a.np = np; a.nw = nw; a.cell = cell;
    a.lcell = cell_log2(cell);
    a.nq = (uint32_t)nq;
    k_ffa_search<<<grid, dim3(kFfaThreads), 0, (hipStream_t)stream>>>(prof, rstd, rm, snr, code, phase, a);
    LAUNCHCHK();
    return PSS_OK;
}

}  // extern "C"
