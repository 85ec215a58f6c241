#pragma once
// pss_plan.hpp -- the host side of a pss_run: the kernel parameter block, the
// length classification that picks a path, the workspace layout, the fast-path
// predicates and the entry points of the launch units.  No kernel lives here.
//
// One PssPipeline run = source -> [FFT delay ramp] -> [null] -> [noise] -> data.
// See include/pss_hip.h for the ABI and DESIGN.md for the kernel/roofline
// discussion.  Paths (run_paths, pss_pipeline.hip):
//   * no delay stage           : k_elementwise          (1 HBM pass)
//   * N = 2^m, 64 <= N <= 8192 : k_single<L>            (1 HBM pass, FFT in LDS)
//   * N = 2^m, N >= 16384      : pair-mode four-step, two channels per complex
//                                row: k_pairA -> k_pair_row -> k_pairC (2 spills)
//   * 2^m x {6..60} (smooth)   : mixed-radix four-step
//   * other even N <= 8192     : direct DFT              (O(N^2) in LDS tiles)
//   * other even N >  8192     : Bluestein chirp-z through a 2^m four-step
#include <string.h>
#include <algorithm>

#include "pss_common.hpp"

using namespace pss;

// ---------------------------------------------------------------------------
// opt-in per-kernel timing and the launch-plan log (defined in pss_pipeline.hip)
// ---------------------------------------------------------------------------
enum { TK_ELEM = 0, TK_SINGLE, TK_COLA, TK_ROW, TK_COLC, TK_FALLBACK, TK_NULLFIX, TK_N };
void tk_begin(int kind, hipStream_t st);
void tk_end(hipStream_t st);
// launch-plan log (pss_plan_collect): every launch path notes the kernels it
// picked ("fourstep 1024x4096 A:fast R:pair_row C:fast N:fix_list"; C:null: the
// fast pass C nulled the always-nulled samples, N:fix_list the rest), so the
// parity tests can assert which kernels produced the bits they check
void plan_note(const char *fmt, ...);

// ---------------------------------------------------------------------------
// kernel parameters
// ---------------------------------------------------------------------------
struct KP {
    PssPipeline p;
    int64_t N;      // samples per row
    int64_t N1;     // four-step: column length (1 for single-pass)
    int64_t N2;     // four-step: row length    (N for single-pass)
    float invN;
    // four-step pair mode (two channels per complex row)
    int npairs;
    int poff;       // chan0 & 1: pairs are (even, odd) GLOBAL channels
    cf *Yd;         // data pair spill    [npairs][N1][sp]
    cf *Ym;         // node pair spill    [KCH/2][N1][N2] (mask table build)
    const cf *Mspec;// mask spectrum      [N1][N2] (natural k2 per row k1)
    // delayed-null mask table (four-step lengths; see k_mask_table)
    int mtab;               // 1: mask decisions come from the table
    int log2n;
    const uint2 *mt_bits;   // [N/32] {nulled-for-every-f bits, f-dependent bits}
    const uint32_t *mt_base;// [N/32] index of the word's first f-dependent position
    const float *mt_coef;   // [n_f_dependent][KCH] root records of the f-dependent positions (root_hit)
    const uint32_t *mbits;  // [nchan][N/32] per-channel null decisions (k_mask_bits)
    int mbB;                // column-block width B of pass C (mbits layout)
    const cf *rtab;         // [npairs][RFL][2] row-pass pair ramp factors {E, D} (k_pair_tab)
    hipEvent_t mask_ready;  // mask table built on a side stream: wait before its first use (or NULL)
    const uint32_t *wlist;  // delayed null: table words with a nulled position (any f)
    const uint32_t *nwlist; // its length (device)
    // single-workgroup kernel with a float64-refined delayed null: the
    // inverse transform's (data, mask) pairs go to this [nchan][N] buffer
    // (the packed paths' W1) instead of through the epilogue
    cf *w1_out;
    // shared-profile fast pass A: the pulse profile at every sample, in the
    // pass's item order (k_prof_cols, PairCols::prof_cols)
    const float4 *pcol;
};
// pair spill row pitch and per-pair stride (complex)
__host__ __device__ __forceinline__ int64_t rpitch(const KP &k) { return k.N2; }
__host__ __device__ __forceinline__ int64_t pstride(const KP &k) { return k.N1 * rpitch(k); }

// node shifts of the delayed-null mask table (the comment above mask_split,
// pss_stages.hpp): here because the workspace holds KCH node rows
static constexpr int KCH = 12;
// floats per f-dependent position record (root_hit): 16 (64 B, aligned)
static constexpr int KREC = 16;
// PCHIP intervals the fast pass A keeps in LDS (two rows; 69.7 KB FFT buffer +
// 12 KB still allows two 512-thread workgroups per CU): a bound of fast_source
static constexpr int kFastNint = 376;

// ---------------------------------------------------------------------------
// length classification
// ---------------------------------------------------------------------------
static inline bool fourstep_len(int64_t n) { return is_pow2(n) && n >= 16384 && n <= (1ll << 24); }
// The power-of-two four-step's N = N1 x N2 (columns x rows; run_fourstep and
// run_fourstep_b launch the kernels of the split this returns):
//   2^14 .. 2^16 : 16 columns, rows of N / 16
//   2^17 .. 2^22 : rows of 4096 (two rows of a pair in 66 KB of LDS), N / 4096 columns
//   2^23         : 1024 x 8192
//   2^24         : 1024 x 16384 for a plain delay (C5: one-row-at-a-time row
//                  pass); with a delayed null (the mask table's row engine
//                  holds a pair of rows), a transfer function or the tail
//                  (`plain` false): 2048 x 8192
static inline bool fourstep_split(int64_t n, bool plain, int64_t *N1 = nullptr, int64_t *N2 = nullptr) {
    if (!fourstep_len(n)) return false;
    int64_t n2 = 4096;
    if (n == (1ll << 24)) n2 = plain ? 16384 : 8192;
    else if (n == (1ll << 23)) n2 = 8192;
    else if (n < (1ll << 17)) n2 = n / 16;
    if (N1) *N1 = n / n2;
    if (N2) *N2 = n2;
    return true;
}

// Mixed-radix four-step lengths: even N = N1 * N2 with N2 = 2^m in
// [1024, 8192] (the largest such power that leaves N1 even) and N1 one of the
// {2, 3, 4, 5}-smooth column lengths below (e.g. the fold-mode C4 length
// 30720 = 30 x 1024).  Other even lengths take the direct path.
static inline bool smooth_col(int64_t n1) {
    switch (n1) {
        case 6: case 10: case 12: case 20: case 24: case 30: case 40: case 48: case 60: return true;
        default: return false;
    }
}
// 5-smooth lengths with few factors of two take an LDS four-step with
// radix-5 stages both ways: 3 125 000 = 2^3 5^8 (the sample count of the
// reference's own simulate fixture, tests/test_simulate.py:47-56) as 1250
// columns (2 x 5^4) x rows of 2500 (4 x 5^4).
static inline bool smooth5_split(int64_t n, int64_t *N1 = nullptr, int64_t *N2 = nullptr) {
    if (n != 3125000) return false;
    if (N1) *N1 = 1250;
    if (N2) *N2 = 2500;
    return true;
}
static inline bool smooth_split(int64_t n, int64_t *N1 = nullptr, int64_t *N2 = nullptr) {
    if (smooth5_split(n, N1, N2)) return true;
    if (n <= 0 || (n & 1) || is_pow2(n) || n > (1ll << 24)) return false;
    int v2 = __builtin_ctzll((unsigned long long)n);
    const int m = v2 - 1 < 13 ? v2 - 1 : 13;            // keep N1 even
    if (m < 10) return false;
    const int64_t n2 = 1ll << m, n1 = n / n2;
    if (!smooth_col(n1)) return false;
    if (N1) *N1 = n1;
    if (N2) *N2 = n2;
    return true;
}

extern int g_flags;   // pss_set_flags (test hook), pss_pipeline.hip

// Bluestein geometry of a fallback length N > 8192 (path 3b): M = M1 x M2,
// nb channels per convolution batch (the batch buffer is about one W buffer).
struct BsGeom { int64_t M, M1, M2, nb; };
static inline bool bs_len(int64_t N) { return N > 8192 && N <= (1ll << 24); }
static inline BsGeom bs_geom(int32_t nchan, int64_t N) {
    BsGeom g;
    g.M = 1;
    while (g.M < 2 * N - 1) g.M <<= 1;
    g.M2 = g.M >= (1ll << 25) ? 8192 : 4096;
    g.M1 = g.M / g.M2;
    g.nb = ((int64_t)nchan * N + g.M - 1) / g.M;    // (ceil: no near-empty last batch)
    if (g.nb < 1) g.nb = 1;
    if (g.nb > nchan) g.nb = nchan;
    if (g.nb > 65535) g.nb = 65535;
    return g;
}

// The plan of a delay-stage run (pss_plan_geometry, include/pss_hip.h), in
// the order run_paths tries the paths -- run_paths dispatches on the kind
// this returns, and the launchers take N1 x N2 from the same split functions.
static inline int plan_variant(const PssPipeline &p) {
    return p.null_mode == PSS_NULL_DELAYED ? 1 : (p.htab || p.tail_a) ? 2 : 0;
}
static inline int plan_geometry(int64_t N, int variant, int64_t *N1 = nullptr, int64_t *N2 = nullptr) {
    int64_t n1 = 0, n2 = 0;
    int kind = PSS_PLAN_DIRECT;
    if (N <= 0 || (N & 1) || (N > (1ll << 24) && !is_pow2(N))) {
        kind = PSS_PLAN_UNSUPPORTED;                 // (validate() rejects these)
    } else if (is_pow2(N) && N >= 64 && N <= 8192) {
        kind = PSS_PLAN_SINGLE;
        n1 = 1;
        n2 = N;
    } else if (fourstep_split(N, variant == 0, &n1, &n2)) {
        kind = PSS_PLAN_FOURSTEP;
    } else if (variant != 1 && smooth_split(N, &n1, &n2)) {
        kind = PSS_PLAN_SMOOTH;                      // (a delayed null off 2^m: the packed paths)
    } else if (bs_len(N) && !(g_flags & PSS_FLAG_DIRECT_DFT)) {
        const BsGeom g = bs_geom(1, N);
        kind = PSS_PLAN_BLUESTEIN;
        n1 = g.M1;
        n2 = g.M2;
    }
    if (N1) *N1 = n1;
    if (N2) *N2 = n2;
    return kind;
}

static constexpr int64_t kRefineMaxN = 1 << 17;
static constexpr int kBsParts = 16;
// refine candidate list capacity (entries of 8 B): 1/8 of the samples + 64 Ki
// (C4's fold-mode geometry with a null has ~7 % candidates: its boxes are
// chi2(Nfold ~ 1e4) values, so the band is ~0.3 wide and the boxes' Gibbs
// ringing crosses it often)
static inline int64_t refine_cap(int32_t nchan, int64_t N) {
    const int64_t all = (int64_t)nchan * N;
    return std::min<int64_t>(all, all / 8 + 65536);
}

// ---------------------------------------------------------------------------
// workspace layout (every region 256-B aligned)
//   four-step (N = 2^m, 2^14 <= N <= 2^24):
//     Yd [npairs][N] cf | Mspec [N] cf | node spill [KCH/2][N] cf |
//     nodes [KCH][N] f32 | table bits [N/64] uint4 | base [N/64] u32 |
//     coef [N][KREC] f32 (worst case) | misc (counter, node ramps/nyq) |
//     null bits [nchan][N/32] u32 | mask row [N] f32
//   single pass (N <= 8192): mask row
//   direct DFT fallback: W1, W2 [nchan][N] cf | twiddles [N] cf | mask row
// ---------------------------------------------------------------------------
struct WsLayout {
    int64_t yd, mspec, ynode, nodes, bits, base, coef, misc, mbits, rtab, wlist, row, total;
    int64_t bs_chirp, bs_bhat, bs_z;   // Bluestein: w [N] | Bhat [M] | Z [nb][M] (cf)
    int64_t odd_tw;                    // odd N: exp(+2 pi i j / (N - 1)), j < N - 1 (cf)
    int64_t rf_tw, rf_B, rf_mx;        // float64 null decisions: e^{2 pi i n/N} [N], B [N/2+1] (double2), row max [nchan]
    int64_t rf_part, rf_list, rf_cnt;  // ... partial spectra [kBsParts][N/2+1] (double2), candidate list, its count
    int64_t pcol;                      // four-step: the profile at every sample (float4 items, k_prof_cols)
    // four-step: the table words with an f-dependent position (k_mask_words'
    // second list: the fix-up after a pass C that nulled the always-nulled
    // samples) and its count.  The list takes the node rows' bytes -- their
    // last reader, k_mask_table, is ahead of k_mask_words on its stream -- and
    // the count a word of misc, so the workspace keeps its size.
    int64_t wlist_f, wcount_f;
};

static inline WsLayout ws_layout(int32_t nchan, int64_t N, bool filt = false) {
    WsLayout w;
    memset(&w, 0, sizeof(w));
    int64_t o = 0;
    // the float64 null refine's buffers (launch_null_refine)
    auto refine_bufs = [&] {
        w.rf_tw = o; o += al256(N * 16);
        w.rf_B = o;  o += al256((N / 2 + 1) * 16);
        w.rf_mx = o; o += al256((int64_t)nchan * 4);
        w.rf_part = o; o += al256((int64_t)kBsParts * (N / 2 + 1) * 16);
        w.rf_list = o; o += al256(refine_cap(nchan, N) * 8);
        w.rf_cnt = o;  o += 256;
    };
    if (fourstep_len(N)) {
        const int64_t npairs = ((int64_t)nchan + 2) / 2;   // pairs of (even, odd) global channels
        // pair spills: N1 x N2 complex per pair
        const int64_t ps = N;
        w.yd = o;    o += al256(npairs * ps * 8);
        w.mspec = o; o += al256(N * 8);
        w.ynode = o; o += al256((int64_t)(KCH / 2) * ps * 8);
        w.nodes = o; o += al256((int64_t)KCH * N * 4);
        w.bits = o;  o += al256((N / 32) * 8);
        w.base = o;  o += al256((N / 32) * 4);
        w.coef = o;  o += al256(N * KREC * 4);
        w.misc = o;  o += 256;
        w.wlist_f = w.nodes;
        w.wcount_f = w.misc + 12;                              // (misc + 8: the full list's count)
        w.mbits = o; o += al256((int64_t)nchan * (N / 8));   // per-channel null bits
        w.rtab = o;  o += al256(npairs * 2 * 64 * 8);          // row-pass pair ramp factors (RFL <= 64)
        w.wlist = o; o += al256((N / 32) * 4);                 // null fix-up: table words with nulls
        w.pcol = o;  o += al256(N * 4);                        // shared-profile pass A: profile per sample
    } else if (!filt && is_pow2(N) && N >= 64 && N <= 8192) {
        // single-workgroup lengths: W1 [nchan][N] cf and the float64 null
        // refine's buffers (a delayed null: run_single)
        o += al256((int64_t)nchan * N * 8);
        refine_bufs();
    } else {
        // fallback: W1, W2, twiddles -- Bluestein needs W1 only (its forward
        // and inverse DFTs are fused through Z), unless the mixed-radix
        // four-step shares these bytes or the direct DFT is forced
        const bool odd = (N & 1) != 0;
        const bool w1_only = bs_len(N) && !odd && !smooth_split(N) && !(g_flags & PSS_FLAG_DIRECT_DFT);
        o += al256(w1_only ? (int64_t)nchan * N * 8 : 2 * (int64_t)nchan * N * 8 + N * 8);
        if (odd) {
            // odd-length shift_t: twiddles of the (N - 1)-point inverse
            w.odd_tw = o;
            o += al256((N - 1) * 8);
        } else if (bs_len(N)) {
            const BsGeom g = bs_geom(nchan, N);
            w.bs_chirp = o; o += al256(N * 8);
            w.bs_bhat = o;  o += al256(g.M * 8);
            w.bs_z = o;     o += al256(g.nb * g.M * 8);
        }
        if (!odd && N <= kRefineMaxN) refine_bufs();
        if (smooth_split(N)) {
            // mixed-radix four-step (inside the same bytes: the direct path
            // still serves these lengths for a delayed null)
            const int64_t npairs = ((int64_t)nchan + 2) / 2;
            w.yd = 0;
            w.rtab = al256(npairs * N * 8);
            w.pcol = o; o += al256(N * 4);
        }
    }
    w.row = o;
    o += al256(N * 4);
    w.total = o;
    return w;
}

// The float64 null decisions of the packed paths (k_null_refine): the
// direct / Bluestein rows and the single-workgroup kernel's, between the
// inverse transform (W1 = data + i mask per row) and the epilogue.
static inline bool refine_null(const KP &k) {
    return k.p.null_mode == PSS_NULL_DELAYED && (k.N & 1) == 0 && k.N <= kRefineMaxN && !k.p.tail_a &&
           !k.p.htab && !(g_flags & PSS_FLAG_NULL_F32);
}

// Fast-path selection (kernels specialised for the north-star configuration;
// results are bitwise identical to the generic kernels).

static inline bool fast_source(const PssPipeline &p) {
    if (g_flags & PSS_FLAG_NO_FAST) return false;
    // (nint == knot_m: the table spans the period, so the fast walk needs no
    // extrapolation clamp -- pulsar._device_table always builds it so)
    return p.src == PSS_SRC_SEARCH && !p.gen_amp && p.gen_df == 1.0f && !p.inj_gen && p.null_mode != PSS_NULL_UNDELAYED &&
           p.nint <= kFastNint && !p.prof_split && (uint32_t)p.nint == p.knot_m;
}
// Fold-mode fast passes of the mixed-radix split (PairCols::passA_fold /
// passC_fold): the fold source with chi2(df != 1) pair draws, and an
// epilogue of noise only (any df != 1), no injected draws.
static inline bool fold_source(const PssPipeline &p) {
    if (g_flags & PSS_FLAG_NO_FAST) return false;
    return p.src == PSS_SRC_FOLD && !p.gen_amp && !p.inj_gen && p.gen_df != 1.0f && p.nph > 0 &&
           p.null_mode != PSS_NULL_UNDELAYED;
}
static inline bool fold_epilogue(const KP &k) {
    const PssPipeline &p = k.p;
    if (g_flags & PSS_FLAG_NO_FAST) return false;
    if (p.out_kind != PSS_OUT_NONE || p.inj_noise || p.inj_rep) return false;
    return p.noise && p.noise_df != 1.0f && p.null_mode != PSS_NULL_DELAYED;
}
static inline bool fast_epilogue(const KP &k) {
    const PssPipeline &p = k.p;
    if (g_flags & PSS_FLAG_NO_FAST) return false;
    if (p.out_kind != PSS_OUT_NONE || p.inj_noise || p.inj_rep) return false;
    if (!p.noise || p.noise_df != 1.0f) return false;
    if (p.null_mode == PSS_NULL_UNDELAYED) return false;
    if (p.null_mode == PSS_NULL_DELAYED && (!k.mtab || p.null_rep_df != 1.0f)) return false;
    return on_grid16(p.data, p.ld);
}

// ---------------------------------------------------------------------------
// entry points of the launch units (one translation unit each, compiled in
// parallel: psrsigsim_amd/build.py)
// ---------------------------------------------------------------------------
int launch_elementwise(const KP &k, hipStream_t st);              // pss_pipeline.hip
int launch_box_row(const KP &k, float *row, hipStream_t st);      // pss_pipeline.hip
// (fdep: pass C nulled the always-nulled samples; only the f-dependent hits are left)
int launch_null_fix(const KP &k, hipStream_t st, bool fdep);      // pss_fourstep.hip
int run_fourstep(KP &k, hipStream_t st, const float *mask_row);   // pss_fourstep.hip
int run_smooth(KP &k, hipStream_t st);                            // pss_smooth.hip (N1 = 6 .. 20)
int run_smooth_b(KP &k, hipStream_t st);                          // pss_smooth_b.hip (N1 = 24, 30, 40)
int run_smooth_c(KP &k, hipStream_t st);                          // pss_smooth_c.hip (N1 = 48, 60; 1250 x 2500)
int run_fourstep_b(KP &k, hipStream_t st, const float *mask_row); // pss_fourstep_b.hip (N != 2^22)
int run_single(KP &k, hipStream_t st);                            // pss_single.hip
int run_fallback(KP &k, hipStream_t st);                          // pss_fallback.hip
int launch_null_refine(KP &k, hipStream_t st);                    // pss_fallback.hip
int launch_fb_epilogue(KP &k, hipStream_t st);                    // pss_fallback.hip
int shift_rows_odd(float *rows, int32_t nrows, int64_t n, int64_t ld, const uint64_t *ramp, void *work,
                   hipStream_t st);                               // pss_fallback.hip
// the mask-table template's (build_mask_table) non-template kernels, launched
// through pss_fourstep.hip (each kernel is compiled in one unit only)
int launch_node_params(uint64_t *ramp, float *nyq, int L, hipStream_t st);
int launch_mask_table(const float *nodes, int64_t N, uint2 *bits, uint32_t *base, float *coef, uint32_t *counter,
                      hipStream_t st);
int launch_mask_words(const uint2 *bits, uint32_t nwords, uint32_t *list, uint32_t *count, uint32_t *list_f,
                      uint32_t *count_f, hipStream_t st);
int launch_mask_bits(const KP &k, uint32_t *bm, hipStream_t st);
