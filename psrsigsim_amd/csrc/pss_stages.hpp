#pragma once
// pss_stages.hpp -- the per-sample device code every synthesis path shares:
// the delayed-null mask-table lookups, the source stage (profile x draws, the
// box mask), the epilogue (null replacement, the observe() copy, noise, store)
// and the delay ramp of a frequency bin.  No kernel lives here; the paths'
// kernels call these between their own loads, transforms and stores.
#include <math.h>
#include <type_traits>

#include "pss_plan.hpp"

// compile-time loop: f(std::integral_constant<int, I>) for I in [B, E)
template <int B, int E, typename F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        static_for<B + 1, E>(f);
    }
}

// ---------------------------------------------------------------------------
// Delayed-null mask table.
//
// The reference shifts ONE box row (the same for every channel) by each
// channel's total delay s_c and nulls where the result exceeds 1
// (pulsar.py:306-330).  Write s = i + f (i integer, f in [0,1)).  For integer
// sample offsets d the shift_t kernel, Nyquist rule included, satisfies
// h_s(d) = h_f(d - i): the integer part is an exact circular roll, so
//     mask_c[n] = M(p, f_c),  p = (n - i_c) mod N,
// with M(p, f) = shift_t(box, f)[p] one function of (p, f) for all channels.
// As a function of f, M(p, .) is a trigonometric polynomial of bandwidth
// pi (bins |k| <= N/2), so a degree-11 Chebyshev interpolant in t = 2f - 1
// from KCH = 12 node shifts is exact to ~1e-9 relative (tools: DESIGN.md §3).
// Per position the table stores whether M > 1 for EVERY f (bound
// c0 -+ sum|c_n|), for NO f, or -- for the ~2% of positions near box edges
// where the answer depends on f -- the f values (as t) where the fp32
// interpolant crosses 1, found once per position by the table build
// (root_hit; the per-channel lookup is then two compares).  The node shifts are
// KCH/2 pair rows through the same FFT engine, once per run; per channel
// nothing but a table lookup remains (no per-channel mask FFT or spill).
// (KCH and KREC, the record size, are defined with the workspace: pss_plan.hpp.)
// ---------------------------------------------------------------------------
// t = 2 f - 1 and i from the mask ramp word w = frac(s / N) 2^64 (N = 2^L)
__device__ __forceinline__ void mask_split(uint64_t w, int L, uint32_t &ishift, float &t) {
    ishift = (uint32_t)(w >> (64 - L));
    const uint64_t fr = w << L;                         // f in 2^-64 units
    t = fmaf((float)(uint32_t)(fr >> 40), 1.1920928955078125e-07f, -1.0f);   // 2 f - 1
}

// Clenshaw evaluation of the degree-11 Chebyshev interpolant at t (the mask
// value M(p, f), t = 2 f - 1), fp32: the table build's root scan uses it
__device__ __forceinline__ float cheb_eval_r(const float4 (&q)[3], float t) {
    const float4 a = q[0], b = q[1], d = q[2];
    const float cc[KCH] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, d.x, d.y, d.z, d.w};
    const float t2 = 2.0f * t;
    float b1 = 0.f, b2 = 0.f;
#pragma unroll
    for (int n = KCH - 1; n >= 1; --n) {
        const float b0 = fmaf(t2, b1, cc[n] - b2);
        b2 = b1;
        b1 = b0;
    }
    return fmaf(t, b1, cc[0] - b2);
}

// Decision of an f-dependent position from its ROOT record (k_mask_table):
// rec = {count, s0, r_1 .. r_10, -}: the fp32 Chebyshev value at t exceeds 1
// iff s0 XOR (the number of roots r_i < t) is odd.  The roots are where
// cheb_eval_r(c, .) > 1 flips, found by a 257-point scan of t in [-1, 1]
// (24 bisection steps per flip) whose cells are CERTIFIED to hold no hidden
// pair of flips (g = value - 1, D2 = max|g''| <= sum_n |c_n| n^2 (n^2 - 1) / 3
// by Markov's bound on T_n'', fp32 evaluation error included): a cell whose
// ends share a sign holds no root when min(|g(t_j)|, |g(t_j+1)|) > D2 h^2 / 8
// (the chord-interpolation error bound), and one with a sign change holds
// exactly one when the secant |g(t_j+1) - g(t_j)| / h exceeds D2 h (g' keeps
// its sign; ~2 % of the f-dependent positions of C3's mask fail this and keep
// coefficient records, measured with tools/mask_cert.py).  The rule then reproduces the direct
// evaluation except within ~1e-8 of a flip, with one 16-B load and two
// compares per position instead of 48 B of coefficients and a 12-term
// Clenshaw sum; unused roots are +inf.  A position whose cells cannot all be
// certified keeps its coefficients instead: rec = {-1, -, -, -, c_0 .. c_11},
// evaluated directly.  `a` is the record's first float4.
__device__ __forceinline__ bool root_hit(const float4 a, const float *rec, float t) {
    if (a.x < 0.f) {                     // uncertified: the coefficient record
        const float4 q[3] = {reinterpret_cast<const float4 *>(rec)[1], reinterpret_cast<const float4 *>(rec)[2],
                             reinterpret_cast<const float4 *>(rec)[3]};
        return cheb_eval_r(q, t) > 1.0f;
    }
    bool h = (a.y != 0.f) ^ (t > a.z) ^ (t > a.w);
    if (a.x > 2.f) {                    // rare: more than two flips over f in [0, 1)
        const float4 b = reinterpret_cast<const float4 *>(rec)[1], c = reinterpret_cast<const float4 *>(rec)[2];
        h ^= (t > b.x) ^ (t > b.y) ^ (t > b.z) ^ (t > b.w) ^ (t > c.x) ^ (t > c.y) ^ (t > c.z) ^ (t > c.w);
    }
    return h;
}

// Null decision bits (bit i: sample n0 + i) for 4 consecutive samples of a
// channel with mask split (ishift, t): a 4-bit window of the two table words
// covering positions p0..p0+3 (mod N), branch-free; the Chebyshev evaluation
// only where a position's decision depends on f (~2% of positions).
__device__ __forceinline__ uint32_t mask_hits4(const KP &k, int64_t n0, uint32_t ishift, float t) {
    const uint32_t nm = (uint32_t)k.N - 1u;
    const uint32_t p0 = ((uint32_t)n0 - ishift) & nm;
    const uint32_t w = p0 >> 5, w2 = (w + 1u) & (nm >> 5), sh = p0 & 31u;
    const uint2 A = k.mt_bits[w], Bw = k.mt_bits[w2];
    uint32_t r = (uint32_t)(((((uint64_t)Bw.x) << 32) | A.x) >> sh) & 15u;
    const uint32_t amb = (uint32_t)(((((uint64_t)Bw.y) << 32) | A.y) >> sh) & 15u;
    if (amb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if ((amb >> i) & 1u) {
                const uint32_t p = (p0 + (uint32_t)i) & nm, pw = p >> 5;
                const uint32_t word = (pw == w) ? A.y : Bw.y;
                const uint32_t idx = k.mt_base[pw] + (uint32_t)__popc(word & ((1u << (p & 31u)) - 1u));
                const float *rec = k.mt_coef + (int64_t)idx * KREC;
                const bool hit = root_hit(reinterpret_cast<const float4 *>(rec)[0], rec, t);
                r = (r & ~(1u << i)) | ((uint32_t)hit << i);
            }
        }
    }
    return r;
}

// Null decisions of the RUN <= 32 contiguous samples n .. n + RUN - 1 of a
// channel with mask split (is, t): a window of the two table words covering
// them; the Chebyshev evaluation only at f-dependent positions (~2%).
__device__ __forceinline__ uint32_t mask_run(const KP &k, uint32_t n, uint32_t is, float t, uint32_t RUN) {
    const uint32_t nm = (uint32_t)k.N - 1u, wm = nm >> 5;
    const uint32_t p0 = (n - is) & nm, w = p0 >> 5, w2 = (w + 1u) & wm, sh = p0 & 31u;
    const uint2 A = k.mt_bits[w], Bw = k.mt_bits[w2];
    const uint32_t msk = RUN >= 32u ? 0xffffffffu : ((1u << RUN) - 1u);
    uint32_t r32 = (uint32_t)(((((uint64_t)Bw.x) << 32) | A.x) >> sh) & msk;
    uint32_t amb = (uint32_t)(((((uint64_t)Bw.y) << 32) | A.y) >> sh) & msk;
    if (!amb) return r32;
    // Ambiguous positions cluster at pulse edges (a lane may hold ~20): take
    // them four at a time so the coefficient loads of a group are in flight
    // together instead of one exposed latency per position (the table bases
    // of the two words are loaded once).
    const uint32_t baseA = k.mt_base[w], baseB = k.mt_base[w2];
    while (amb) {
        uint32_t ii[4], idx[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            ii[u] = amb ? (uint32_t)__ffs(amb) - 1u : 32u;
            amb &= amb - 1u;
            const uint32_t p = (p0 + (ii[u] & 31u)) & nm;
            const bool inA = (p >> 5) == w;
            const uint32_t word = inA ? A.y : Bw.y;
            idx[u] = (inA ? baseA : baseB) + (uint32_t)__popc(word & ((1u << (p & 31u)) - 1u));
        }
        float4 a[4];
        const float *rec[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            rec[u] = k.mt_coef + (int64_t)(ii[u] < 32u ? idx[u] : idx[0]) * KREC;
            a[u] = reinterpret_cast<const float4 *>(rec[u])[0];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (ii[u] < 32u) {
                const bool hit = root_hit(a[u], rec[u], t);
                r32 = (r32 & ~(1u << ii[u])) | ((uint32_t)hit << ii[u]);
            }
        }
    }
    return r32;
}

// 4 null decisions of channel row r for samples n1 N2 + n20 + b4 .. + 3.
// (column block blockIdx.x of B columns, N1 rows; B, N1 as in pass C)
template <int B, int N1>
__device__ __forceinline__ uint32_t mask_bits4(const KP &k, int r, int cbx, int n1, int b4) {
    const uint32_t bp = (((uint32_t)cbx * (uint32_t)N1 + (uint32_t)n1) * (uint32_t)B) + (uint32_t)b4;
    return (k.mbits[(int64_t)r * (k.N >> 5) + (bp >> 5)] >> (bp & 31u)) & 15u;
}

// XCD-aware block order of the column passes.  Workgroups are dispatched
// round-robin over the 8 XCDs (linear id % 8), each with its own L2; the
// passes touch B-column segments of every row (32 B of fp32 output per channel
// for B = 8, a quarter of a 128-B line).  Remapping linear id ->
// (id % 8) * (total / 8) + id / 8 gives each XCD a contiguous range of column
// blocks, so the pieces of a line are written through the same L2 at about the
// same time and merge there.  Measured (pass C, 2048 x 2^22): 17.8-19 ms with
// the remap, 61 ms without, 58 ms with the blocks bit-reversed over the row;
// contiguous (wrong-place) stores would take 14.3 ms -- the residual cost of
// the strided output is ~4 ms.  Non-temporal / sc1 loads of the spill make it
// worse (21-25 ms): neighbouring blocks share the spill's lines through L2.
// (Only grids that are a multiple of 8 are remapped; xcd_run_id, pss_common.hpp,
// is the stand-alone stages' 1-D map for any grid.)
__device__ __forceinline__ void xcd_block(int &bx, int &by) {
    const uint32_t gx = gridDim.x, total = gx * gridDim.y;
    const uint32_t id = blockIdx.x + blockIdx.y * gx;
    const uint32_t l = ((total & 7u) == 0u) ? (id & 7u) * (total >> 3) + (id >> 3) : id;
    by = (int)(l / gx);
    bx = (int)(l - (uint32_t)by * gx);
}

__device__ __forceinline__ int64_t floordiv(int64_t a, int64_t b) {
    int64_t q = a / b;
    if ((a % b != 0) && ((a < 0) != (b < 0))) --q;
    return q;
}

// Box (nulled pulse) covering sample n, following the reference's numpy
// indexing: bins = arange(Nph p, Nph (p+1)) + shift_val, filtered < N; negative
// bins address from the end; later pulses in the choice list overwrite.
__device__ __forceinline__ bool box_of(const KP &k, int64_t n, int &rank, int &j) {
    const PssPipeline &p = k.p;
    rank = -1;
    const int64_t nph = p.nph;
    const int64_t shift = p.null_shift_dev ? *p.null_shift_dev : p.null_shift;
    int64_t q = n - shift;
    int64_t s = floordiv(q, nph);
    if (s >= 0 && s < p.null_slots) {
        int r = p.null_rank[s];
        if (r >= 0) { rank = r; j = (int)(q - s * nph); }
    }
    q = n - k.N - shift;                 // the same sample reached by a negative bin
    s = floordiv(q, nph);
    if (s >= 0 && s < p.null_slots) {
        int r = p.null_rank[s];
        if (r > rank) { rank = r; j = (int)(q - s * nph); }
    }
    return rank >= 0;
}

__device__ __forceinline__ float box_value(const KP &k, int64_t n, int rank, int j) {
    const PssPipeline &p = k.p;
    if (p.inj_box) return p.inj_box[n];
    Rng g(p.seed, p.call_null, P_BOX);
    return chi2_general(g, (uint32_t)j, (uint32_t)rank, p.null_box_df) * p.null_box_scale;
}

// chi2 draws for 4 consecutive samples n0..n0+3 (n0 % 4 == 0) of channel c.
// df == 1: one Philox block per 4 samples; otherwise the Marsaglia-Tsang
// pair sampler, one shared block per 2 samples (chi2_pair).
__device__ __forceinline__ void draw4(const Rng &g, int64_t n0, uint32_t c, float df, float (&x)[4]) {
    if (df == 1.0f) {
        float4 q = chi2_1x4(g.bits((uint32_t)(n0 >> 2), c, (uint32_t)(n0 >> 34)));
        x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
    } else {
        const uint32_t m = (uint32_t)(n0 >> 1);
        chi2_pair(g, m, c, df, x[0], x[1]);
        chi2_pair(g, m + 1u, c, df, x[2], x[3]);
    }
}

// Interval index and fraction of sample n's pulse phase (shared by every
// channel: only the coefficient row differs).
__device__ __forceinline__ void pchip_locate(const KP &k, int64_t n, uint32_t &iv, float &u) {
    const PssPipeline &p = k.p;
    // ph = n * phase_step mod 2^64 (2^-64 cycles), n < 2^32: 32-bit products only
    const uint32_t nn = (uint32_t)n;
    const uint64_t ph = (uint64_t)nn * (uint32_t)p.phase_step +
                        ((uint64_t)(nn * (uint32_t)(p.phase_step >> 32)) << 32);
    // ph * M = iv 2^64 + fraction; u = (ph * M) >> 32 holds iv and fraction bits 32..63
    const uint64_t t = (uint64_t)(uint32_t)ph * p.knot_m;
    const uint64_t u64 = (uint64_t)(uint32_t)(ph >> 32) * p.knot_m + (t >> 32);
    iv = (uint32_t)(u64 >> 32);                                    // interval index
    u = frac23((uint32_t)u64);                                     // fraction, 23 bits
    if (iv >= (uint32_t)p.nint) {                                  // extrapolate
        u += (float)(iv - (uint32_t)(p.nint - 1));
        iv = p.nint - 1;
    }
}

// The same (interval, fraction) for consecutive samples by increments: the
// 96-bit product A(n) = (n phase_step mod 2^64) * knot_m, kept as three
// 32-bit words (hi = interval field, mid = fraction, lo = guard), advances by
// D = phase_step * knot_m; when the phase wraps the interval field comes back
// by knot_m.  Exact integer arithmetic: bitwise the values pchip_locate
// computes, at one add-with-carry chain and a min per sample (the 64-bit form
// compiled to nine VALU per step) instead of four 32 x 32 -> 64 multiplies.
struct PhaseWalk {
    uint32_t lo, mid, hi;
    __device__ __forceinline__ void start(const PssPipeline &p, uint32_t n) {
        const uint64_t ph = (uint64_t)n * (uint32_t)p.phase_step + ((uint64_t)(n * (uint32_t)(p.phase_step >> 32)) << 32);
        const uint64_t t = (uint64_t)(uint32_t)ph * p.knot_m;
        lo = (uint32_t)t;
        const uint64_t u64 = (uint64_t)(uint32_t)(ph >> 32) * p.knot_m + (t >> 32);
        mid = (uint32_t)u64;
        hi = (uint32_t)(u64 >> 32);
    }
    __device__ __forceinline__ void step(uint32_t dlo, uint64_t dhi, uint32_t M) {
        unsigned c;
        lo = __builtin_addc(lo, dlo, 0u, &c);
        mid = __builtin_addc(mid, (uint32_t)dhi, c, &c);
        hi = hi + (uint32_t)(dhi >> 32) + c;
        // (hi >= M) ? hi - M : hi -- hi < 2 M here, and for hi < M the
        // difference wraps above hi (M <= 2^31)
        hi = min(hi, hi - M);
    }
    // for a table that spans the whole period (nint == knot_m, the host's
    // extrapolated pieces appended: pulsar._device_table), where iv < knot_m
    // needs no clamp -- bitwise what pchip_locate returns then
    __device__ __forceinline__ void get_full(uint32_t &iv, float &u) const {
        iv = hi;
        u = frac23(mid);
    }
};
__device__ __forceinline__ void phase_delta(const PssPipeline &p, uint32_t &dlo, uint64_t &dhi) {
    const uint64_t t = (uint64_t)(uint32_t)p.phase_step * p.knot_m;
    dlo = (uint32_t)t;
    dhi = (uint64_t)(uint32_t)(p.phase_step >> 32) * p.knot_m + (t >> 32);
}

__device__ __forceinline__ float pchip_row(const KP &k, int prow, uint32_t iv, float u) {
    float4 cc;
    if (k.p.prof_split) {
        // non-uniform knots: cell iv holds the cubics on either side of its
        // one interior knot (both in the cell coordinate u)
        const float4 *c = reinterpret_cast<const float4 *>(k.p.prof) + ((int64_t)prow * k.p.nint + iv) * 2;
        const float s = k.p.prof[(int64_t)k.p.prof_rows * k.p.nint * 8 + iv];
        cc = (u >= s) ? c[1] : c[0];
    } else {
        cc = reinterpret_cast<const float4 *>(k.p.prof)[(int64_t)prow * k.p.nint + iv];
    }
    return fmaf(fmaf(fmaf(cc.x, u, cc.y), u, cc.z), u, cc.w);
}

__device__ __forceinline__ float pchip_eval(const KP &k, int prow, int64_t n) {
    uint32_t iv;
    float u;
    pchip_locate(k, n, iv, u);
    return pchip_row(k, prow, iv, u);
}

// Analytic Gaussian portrait at sample n's pulse phase (amplitude pulses of
// a GaussProfile / 1-D GaussPortrait, portraits.py:143-178, 277-290):
// prof = [nint components][4] = {peak, 1/width, amp/Amax, 0}, channel
// independent; the phase is pchip_locate's fraction with knot_m = 1.
__device__ __forceinline__ float gauss_eval(const KP &k, int64_t n) {
    uint32_t iv;
    float u;
    pchip_locate(k, n, iv, u);
    const float4 *cp = reinterpret_cast<const float4 *>(k.p.prof);
    float acc = 0.f;
    for (int j = 0; j < k.p.nint; ++j) {
        const float4 c = cp[j];
        const float d = (u - c.x) * c.y;
        acc = fmaf(c.z, __expf(-0.5f * d * d), acc);
    }
    return acc;
}

// Source stage for 4 consecutive samples (cnt valid) of local row r.
// re = data (generated or loaded, with an undelayed null applied);
// im = delayed-null box mask (0 elsewhere).
__device__ __forceinline__ void source4(const KP &k, int r, int64_t n0, int cnt,
                                        float (&re)[4], float (&im)[4], bool want_re,
                                        bool want_im = true) {
    const PssPipeline &p = k.p;
    const uint32_t c = (uint32_t)(p.chan0 + r);
    PSS_DASSERT(r >= 0 && r < p.nchan && n0 >= 0 && n0 + cnt <= k.N);
#pragma unroll
    for (int i = 0; i < 4; ++i) { re[i] = 0.f; im[i] = 0.f; }
    if (want_re) {
        if (p.src == PSS_SRC_LOAD) {
            const float *row = p.data + (int64_t)r * p.ld;
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < cnt) re[i] = row[n0 + i];
        } else {
            float x[4];
            float dn = p.draw_norm;
            if (p.inj_gen) {
                const float *row = p.inj_gen + (int64_t)r * k.N;
#pragma unroll
                for (int i = 0; i < 4; ++i) x[i] = (i < cnt) ? row[n0 + i] : 0.f;
            } else if (p.gen_amp) {
                Rng g(p.seed, p.call_gen, P_PULSE);
                const float4 z = normal_x4(g.bits((uint32_t)(n0 >> 2), c, (uint32_t)(n0 >> 34)));
                x[0] = z.x; x[1] = z.y; x[2] = z.z; x[3] = z.w;
            } else if (p.gen_df == 1.0f) {
                // chi2(1) draws with draw_norm folded into the sampler (as the
                // fast pass A draws them: bitwise the same values)
                // (Philox block n >> 2 holds samples 4 (n >> 2) .. + 3 at every N)
                Rng g(p.seed, p.call_gen, P_PULSE);
                const float4 q = chi2_1x4(g.bits((uint32_t)(n0 >> 2), c, (uint32_t)(n0 >> 34)), p.draw_norm);
                x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
                dn = 1.0f;                                   // (x * 1 is exact)
            } else {
                Rng g(p.seed, p.call_gen, P_PULSE);
                draw4(g, n0, c, p.gen_df, x);
            }
            const int prow = (p.prof_rows == 1) ? 0 : (int)c - p.prof_row0;
            if (p.src == PSS_SRC_SEARCH && p.gen_amp) {
                // amplitude pulses: sqrt(calc_profiles(phase)) x N(0, 1)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i < cnt) {
                        const float pr = (p.gen_amp == 2) ? gauss_eval(k, n0 + i) : pchip_eval(k, prow, n0 + i);
                        re[i] = sqrtf(fmaxf(pr, 0.0f)) * x[i] * dn;
                    }
                }
            } else if (p.src == PSS_SRC_SEARCH) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < cnt) re[i] = pchip_eval(k, prow, n0 + i) * x[i] * dn;
            } else {   // FOLD
                const float *pr = p.prof + (int64_t)prow * p.nph;
                uint32_t b = (uint32_t)(n0 % p.nph);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i < cnt) re[i] = pr[b] * x[i] * dn;
                    if (++b == (uint32_t)p.nph) b = 0;
                }
            }
        }
        if (p.null_mode == PSS_NULL_UNDELAYED) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int rk, j;
                if (i < cnt && box_of(k, n0 + i, rk, j)) re[i] = box_value(k, n0 + i, rk, j);
            }
        }
    }
    if (want_im && p.null_mode == PSS_NULL_DELAYED) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int rk, j;
            if (i < cnt) {
                if (p.inj_box) im[i] = p.inj_box[n0 + i];
                else if (box_of(k, n0 + i, rk, j)) im[i] = box_value(k, n0 + i, rk, j);
            }
        }
    }
}

// observe()'s resampled pre-noise copy (PssPipeline.out_len > 0): the
// samples n0 .. n0 + cnt - 1 of row r added into the float64 sums of the
// windows [lo_j, hi_j) that hold them (down_sample, utils.py:62-68: lo_j =
// j f; rebin, utils.py:71-91: lo_j = ceil(j step), hi_j = ceil(j step + step)
// clipped to N, so neighbouring windows may share a sample).  The edges are
// recomputed from step with the host's float64 operations (out_lo / out_hi
// serve the finalize kernel's counts); a window holding n is floor(n / step)
// or the one before.  A lane's samples form a head piece (its first window)
// and a tail piece (its last; pieces in between go straight to their
// atomics); the head joins the previous lane's tail when they are the same
// window, and the tails are summed over each run of lanes with the same
// window -- a segmented reduction by doubling that only extends a sum over
// lanes it has covered without a gap, and stops once no run is still
// growing -- so one no-return float64 atomic leaves the wave per window
// piece.  (Within-wave sums in fp32: at most 256 samples, summed as a tree.)
// The atomics land in the hardware's order: the pieces are fp32 sums of one
// row's samples, so their float64 sum is exact (order-free) unless a window
// mixes pieces ~2^29 apart in magnitude, and a last-bit difference of the
// float64 mean changes the float32 / int8 result only at a rounding boundary
// (tests/test_gpu_observe_resample.py: two identical runs, the same bits).
// Waves whose lanes hold different rows (the single-workgroup kernel's row
// batches) skip the cross-lane step.  k_out_finalize divides, clips and casts
// (telescope.py:140-145).  All active lanes of a wave call it together (the
// epilogues' item loops are wave-uniform up to their tails; inactive lanes
// are masked out through the ballot).
__device__ __forceinline__ void out_windows(const PssPipeline &p, int r, uint32_t N, uint32_t n0, int cnt,
                                            const float (&v)[4]) {
    const int lane = (int)__lane_id();
    const uint64_t act = __ballot(1);
    const uint32_t L = (uint32_t)p.out_len;
    const bool uniform = p.out_lo == nullptr;
    const double step = p.out_step;
    const uint32_t f = (uint32_t)step;
    double *acc = p.out_acc + (int64_t)r * L;
    const uint32_t last = n0 + (uint32_t)cnt - 1u;
    int64_t ja, jb;
    if (uniform) {
        ja = n0 / f;
        jb = last / f;
    } else {
        const double inv = 1.0 / step;      // (wave-uniform: hoisted by the compiler)
        ja = (int64_t)floor((double)n0 * inv) - 2;
        jb = (int64_t)floor((double)last * inv) + 1;
    }
    ja = ja < 0 ? 0 : ja;
    jb = jb > (int64_t)L - 1 ? (int64_t)L - 1 : jb;
    uint32_t jH = 0xffffffffu, jT = 0xffffffffu;      // head / tail window, ~0: none
    float sH = 0.f, sT = 0.f;
    for (int64_t jj = ja; jj <= jb; ++jj) {
        const uint32_t j = (uint32_t)jj;
        uint32_t lo, hi;
        if (uniform) {
            lo = j * f;
            hi = lo + f;
        } else {
            // two statements: the sum is not contracted into an fma
            const double lb = (double)j * step;
            const double rb = lb + step;
            lo = (uint32_t)ceil(lb);
            hi = (uint32_t)ceil(rb);
            hi = hi > N ? N : hi;
        }
        float s = 0.f;
        bool any = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t n = n0 + (uint32_t)i;
            if (i < cnt && n >= lo && n < hi) {
                s += v[i];
                any = true;
            }
        }
        if (!any) continue;
        if (jT == 0xffffffffu) {
            jH = jT = j;
            sT = s;
        } else {
            if (jH == jT) sH = sT;                            // the first window becomes the head
            else unsafeAtomicAdd(acc + jT, (double)sT);        // a window in the middle of the lane
            jT = j;
            sT = s;
        }
    }
    const bool has_head = jT != 0xffffffffu && jH != jT;
    const int r0 = __builtin_amdgcn_readfirstlane(r);
    if (__ballot(r != r0) != 0ull) {
        // lanes of several rows: no cross-lane merge
        if (has_head) unsafeAtomicAdd(acc + jH, (double)sH);
        if (jT != 0xffffffffu) unsafeAtomicAdd(acc + jT, (double)sT);
        return;
    }
    // the head joins the previous lane's tail (the same window)
    const uint32_t nxt_h = (uint32_t)__shfl_down((int)(has_head ? jH : 0xffffffffu), 1);
    const float nxt_s = __shfl_down(sH, 1);
    const uint32_t prv_t = (uint32_t)__shfl_up((int)jT, 1);
    const bool nxt_ok = lane < 63 && ((act >> (lane + 1)) & 1ull);
    const bool prv_ok = lane > 0 && ((act >> (lane - 1)) & 1ull);
    if (jT != 0xffffffffu && nxt_ok && nxt_h == jT) sT += nxt_s;
    if (has_head && !(prv_ok && prv_t == jH)) unsafeAtomicAdd(acc + jH, (double)sH);
    // segmented sum of the tails over runs of lanes with one window
    const uint32_t key = jT != 0xffffffffu ? jT : 0x80000000u + (uint32_t)lane;   // no tail: a key of its own
    float sum = sT;
    int len = 1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ok_ = (uint32_t)__shfl_down((int)key, d);
        const bool grow = len == d && lane + d < 64 && ((act >> (lane + d)) & 1ull) && ok_ == key;
        if (__ballot(grow) == 0ull) break;
        const float os = __shfl_down(sum, d);
        const int ol = __shfl_down(len, d);
        if (grow) {
            sum += os;
            len += ol;
        }
    }
    if (jT != 0xffffffffu && !(prv_ok && prv_t == key)) unsafeAtomicAdd(acc + jT, (double)sum);
}

// Epilogue for 4 consecutive samples: delayed-null replacement where the
// shifted mask exceeds 1, the observe() pre-noise copy, radiometer noise, store.
// `pre` holds the data value (FFT output already scaled by 1/N, or the source).
__device__ __forceinline__ void epilogue4(const KP &k, int r, int64_t n0, int cnt,
                                          float (&pre)[4], const float (&mask)[4], bool load_data) {
    const PssPipeline &p = k.p;
    const uint32_t c = (uint32_t)(p.chan0 + r);
    float *row = p.data + (int64_t)r * p.ld;
    PSS_DASSERT(r >= 0 && r < p.nchan && n0 >= 0 && n0 + cnt <= k.N);
    if (load_data) {
#pragma unroll
        for (int i = 0; i < 4; ++i) if (i < cnt) pre[i] = row[n0 + i];
    }
    if (p.null_mode == PSS_NULL_DELAYED) {
        const bool any = (mask[0] > 1.0f) | (mask[1] > 1.0f) | (mask[2] > 1.0f) | (mask[3] > 1.0f);
        if (any) {
            float x[4];
            if (p.inj_rep) {
#pragma unroll
                for (int i = 0; i < 4; ++i) x[i] = (i < cnt) ? p.inj_rep[(int64_t)r * k.N + n0 + i] : 0.f;
            } else {
                Rng g(p.seed, p.call_null, P_REP);
                draw4(g, n0, c, p.null_rep_df, x);
#pragma unroll
                for (int i = 0; i < 4; ++i) x[i] *= p.null_rep_scale;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < cnt && mask[i] > 1.0f) pre[i] = x[i];
        }
    }
    if (p.out_kind != PSS_OUT_NONE && p.out_len > 0) {
        out_windows(p, r, (uint32_t)k.N, (uint32_t)n0, cnt, pre);
    } else if (p.out_kind == PSS_OUT_F32) {
        float *o = (float *)p.out + (int64_t)r * k.N;
#pragma unroll
        for (int i = 0; i < 4; ++i) if (i < cnt) o[n0 + i] = (pre[i] > p.clip) ? p.clip : pre[i];
    } else if (p.out_kind == PSS_OUT_I8) {
        int8_t *o = (int8_t *)p.out + (int64_t)r * k.N;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < cnt) {
                float v = (pre[i] > p.clip) ? p.clip : pre[i];
                v = fminf(fmaxf(v, -128.f), 127.f);
                o[n0 + i] = (int8_t)(int)truncf(v);
            }
        }
    }
    if (p.noise) {
        float x[4];
        if (p.inj_noise) {
            const float *nr = p.inj_noise + (int64_t)r * k.N;
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = (i < cnt) ? nr[n0 + i] : 0.f;
        } else {
            Rng g(p.seed, p.call_noise, P_NOISE);
            draw4(g, n0, c, p.noise_df, x);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) pre[i] = fmaf(p.noise_norm, x[i], pre[i]);
    }
    if (cnt == 4 && (((uintptr_t)(row + n0)) & 15) == 0) {
        *reinterpret_cast<float4 *>(row + n0) = make_float4(pre[0], pre[1], pre[2], pre[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) if (i < cnt) row[n0 + i] = pre[i];
    }
}

__device__ __forceinline__ cf apply_ramp_delay(const KP &k, int r, int64_t kb, cf z);

// Scattering-tail transfer function of row r at bin kb (extension, see
// PssPipeline.tail_a): H = (1 - a) / (1 - a e^{-2 pi i kb/N}); exactly 1 at DC
// and real (1-a)/(1+a) at Nyquist, Hermitian in kb, so irfft stays real.
__device__ __forceinline__ cf tail_factor(float a, cf w) {
    // w = e^{-2 pi i kb / N}; 1/(1 - a w) = conj(d) / |d|^2, d = 1 - a w
    const float dr = fmaf(-a, w.x, 1.0f), di = -a * w.y;
    const float s = (1.0f - a) / fmaf(dr, dr, di * di);
    return make_float2(dr * s, -di * s);
}
__device__ __forceinline__ cf bin_phasor(int64_t kb, int64_t N) {
    const int64_t kk = (2 * kb > N) ? kb - N : kb;
    return expi_rev(-(float)((double)kk / (double)N));
}

// exp(-2 pi i k' s / N) for frequency bin k, with the reference's Nyquist
// rule applied separately to the real (data) and imaginary (mask) parts.
__device__ __forceinline__ cf apply_ramp(const KP &k, int r, int64_t kb, cf z) {
    if (k.p.tail_a && !k.p.htab) {
        const cf h = tail_factor(k.p.tail_a[r], bin_phasor(kb, k.N));
        const cf t = apply_ramp_delay(k, r, kb, z);
        if (kb == 0 || 2 * kb == k.N) return make_float2(t.x * h.x, t.y * h.x);   // real parts only
        return cmul(t, h);
    }
    return apply_ramp_delay(k, r, kb, z);
}
__device__ __forceinline__ cf apply_ramp_delay(const KP &k, int r, int64_t kb, cf z) {
    const PssPipeline &p = k.p;
    const int64_t N = k.N;
    if (p.htab) {
        // per-bin transfer function of the rfft bins; Hermitian extension,
        // DC and Nyquist keep Re H only (irfft drops their imaginary parts)
        const bool upper = 2 * kb > N;
        const cf h = reinterpret_cast<const cf *>(p.htab)[upper ? N - kb : kb];
        if (kb == 0 || 2 * kb == N) return make_float2(z.x * h.x, z.y * h.x);
        return cmul(z, make_float2(h.x, upper ? -h.y : h.y));
    }
    if (2 * kb == N) return make_float2(z.x * p.nyq_re[r], z.y * p.nyq_im[r]);
    if (kb == 0) return z;
    const int64_t kk = (2 * kb > N) ? kb - N : kb;
    const uint64_t ph = (uint64_t)kk * p.ramp[r];
    return cmul(z, expi_rev(-fix_to_rev(ph)));
}
