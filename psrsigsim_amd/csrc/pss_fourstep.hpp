#pragma once
// pss_fourstep.hpp -- the four-step kernel templates and their launchers
// (N = N1 x N2: column pass A, row pass, column pass C, two spills), for the
// units that instantiate them: pss_fourstep*.hip (N = 2^m) and pss_smooth*.hip
// (mixed radix).  A change here rebuilds those units only.
#include "pss_stages.hpp"
#include "pss_fft.hpp"

// Fixed product choices (each measured against its alternatives, DESIGN.md
// sections 3 and 10; the rejected variants live in the git history):
//   * column blocks of the column passes mapped XCD-contiguously (xcd_block);
//   * 2^22 split 1024 x 4096 (rows of 4096 for 2^17 .. 2^22), 2^24 split
//     2048 x 8192;
//   * fast pass C, 16-column blocks (64-B output segments) wherever the
//     columns have 1024 points or more: passC_fast32, register-resident
//     columns in 512-thread workgroups -- 1024-point columns (2^22 = C3, 2^23,
//     C5's 1024 x 16384) at the 128-VGPR cap with 72 KB of LDS, two workgroups
//     per CU ("C:fast C:cols16x2"); 2048-point columns (2^24 with a delayed
//     null, 2048 x 8192) at 256 VGPRs, one workgroup per CU ("C:fast32").
//     Shorter columns (2^14 .. 2^21) and the mixed-radix splits: passC_fast,
//     the block in LDS, on pass A's block width ("C:fast");
//   * the delayed-null mask table built on a side stream next to pass A, and
//     applied by the compacted fix-up (k_null_fix_list) after pass C; on
//     1024-point columns pass C itself nulls the samples the table nulls for
//     every f, in its staging ("C:null"), and the fix-up visits only the
//     words with an f-dependent position.

// ---------------------------------------------------------------------------
// path 2: four-step, N = N1 * N2, sample n = N2*n1 + n2, bin k = k1 + N1*k2.
//   A: per (row, block of B columns n2): source, FFT over n1, * W_N^{n2 k1},
//      store Y[row][k1][n2]                                  (work, complex)
//   B: per (row, BR rows k1): FFT over n2 -> ramp(k) -> inverse FFT over k2
//   C: per (row, block of B columns n2): * W_N^{-k1 n2}, inverse FFT over k1,
//      epilogue (null / out / noise), store data[row][N2*n1 + n2]
// The channels run through it in pairs (path 2b below).  One row at a time
// only the forward half is left, A (Cols) and the forward transform of B
// (Rows): the spectrum of the delayed null's mask row (build_mask_table).
// ---------------------------------------------------------------------------
template <int N1, int B, int T, typename FWD>
struct Cols;

template <int N1, int B, int T, int... F>
struct Cols<N1, B, T, RList<F...>> {
    using FF = Fft<N1, B, T>;
    static constexpr int E = FF::E;
    static constexpr int RF0 = FF::template first<F...>();
    static constexpr int RFL = FF::template last_of<F...>();

    __device__ static void passA(const KP &k) {
        __shared__ cf lds[B * Lds<N1>::RS];
        const int tid = threadIdx.x;
        const int r = blockIdx.y;
        const int64_t n20 = (int64_t)blockIdx.x * B;
        const int64_t N2 = k.N2;
        const bool re_in = k.p.data_in_fft != 0;
        for (int it = tid; it < N1 * B / 4; it += T) {
            const int n1 = it / (B / 4);
            const int b4 = (it - n1 * (B / 4)) * 4;
            float re[4], im[4];
            source4(k, r, n1 * N2 + n20 + b4, 4, re, im, re_in);
#pragma unroll
            for (int i = 0; i < 4; ++i) lds[Lds<N1>::at(b4 + i, n1)] = make_float2(re[i], im[i]);
        }
        __syncthreads();
        cf v[E];
        FF::template load<RF0>(v, lds, tid);
        __syncthreads();
        FF::template run<false, 1, F...>(v, lds, tid);
        const float invN = k.invN;
#pragma unroll
        for (int i = 0; i < E; ++i) {
            int b, k1;
            FF::template where<RFL>(i, tid, b, k1);
            int64_t m = (n20 + b) * (int64_t)k1;          // < N
            float rev = (float)m * invN;
            if (rev >= 0.5f) rev -= 1.0f;
            v[i] = cmul(v[i], expi_rev(-rev));
        }
        FF::template store<RFL>(v, lds, tid);
        __syncthreads();
        cf *Y = reinterpret_cast<cf *>(k.p.work) + (int64_t)r * k.N;
        for (int it = tid; it < N1 * B / 4; it += T) {
            const int k1 = it / (B / 4);
            const int b4 = (it - k1 * (B / 4)) * 4;
            cf a0 = lds[Lds<N1>::at(b4 + 0, k1)], a1 = lds[Lds<N1>::at(b4 + 1, k1)];
            cf a2 = lds[Lds<N1>::at(b4 + 2, k1)], a3 = lds[Lds<N1>::at(b4 + 3, k1)];
            float4 *dst = reinterpret_cast<float4 *>(Y + (int64_t)k1 * N2 + n20 + b4);
            dst[0] = make_float4(a0.x, a0.y, a1.x, a1.y);
            dst[1] = make_float4(a2.x, a2.y, a3.x, a3.y);
        }
    }
};

template <typename C, int T>
__global__ __launch_bounds__(T) void k_colA(KP k) { C::passA(k); }

template <int N2, int BR, int T, typename FWD>
struct Rows;

template <int N2, int BR, int T, int... F>
struct Rows<N2, BR, T, RList<F...>> {
    using FF = Fft<N2, BR, T>;
    static constexpr int E = FF::E;
    static constexpr int RF0 = FF::template first<F...>();
    static constexpr int RFL = FF::template last_of<F...>();

    // forward transform of BR rows k1, left in natural k2 order per row (the
    // mask spectrum of pair mode)
    __device__ static void pass(const KP &k) {
        __shared__ cf lds[BR * Lds<N2>::RS];
        const int tid = threadIdx.x;
        const int r = blockIdx.y;
        const int64_t k10 = (int64_t)blockIdx.x * BR;
        cf *Y = reinterpret_cast<cf *>(k.p.work) + (int64_t)r * k.N + k10 * N2;
        cf v[E];
        constexpr int LR = N2 / RF0;
#pragma unroll
        for (int ib = 0; ib < E / RF0; ++ib) {
            const int j = tid + ib * T, b = j / LR, jj = j - b * LR;
#pragma unroll
            for (int q = 0; q < RF0; ++q) v[ib * RF0 + q] = Y[(int64_t)b * N2 + jj + q * LR];
        }
        FF::template run<false, 1, F...>(v, lds, tid);
#pragma unroll
        for (int i = 0; i < E; ++i) {
            int b, k2;
            FF::template where<RFL>(i, tid, b, k2);
            Y[(int64_t)b * N2 + k2] = v[i];
        }
    }
};

template <typename R, int T>
__global__ __launch_bounds__(T) void k_row(KP k) { R::pass(k); }

// ---------------------------------------------------------------------------
// path 2b: four-step in PAIR mode.  Two channels a = 2p, b = 2p+1 share one
// complex row z = d_a + i d_b (half the spill bytes and half the column FFTs).
// The row pass separates their spectra with the Hermitian pairing
//   D_a(k) = (Z(k) + conj Z(N-k)) / 2,   D_b(k) = (Z(k) - conj Z(N-k)) / 2i,
// bin N-k of row k1 living in row N1-k1 (column N2-1-k2; row 0 and N1/2 pair
// with themselves), applies each channel's ramp and recombines
// W = D_a R_a + i D_b R_b before the inverse.  A delayed-null mask (same row
// for every channel) is transformed once per run (Mspec) and turned into the
// pair V = M R'_a + i M R'_b by the row pass, spilled, and inverted by pass C
// next to the data.
// ---------------------------------------------------------------------------
// Ramps in the row pass.  A thread's last-stage (radix RFL) group holds bins
// kb = kb0 + q N/RFL (q < RFL, kb0 < N/RFL); the reference's phase
// kb' s / N (kb' = kb - N above N/2) is, in 64-bit fixed point,
//   kb0 w + q (N/RFL) w - [2q >= RFL] N w   (mod 2^64, w = ramp word),
// so per bin only a 64-bit add of a uniform (scalar) offset is needed --
// bit-identical to multiplying kb' w directly.
template <int RFL>
__device__ __forceinline__ cf ramp_q(uint64_t p0, uint64_t step, uint64_t nw, int q) {
    uint64_t ph = p0 + (uint64_t)q * step;
    if (2 * q >= RFL) ph -= nw;                 // q is a compile-time constant here
    return expi_rev(-fix_to_rev(ph));
}

// Pair form of the ramps.  With R_a = e^{-2 pi i k' w_a / 2^64} and R_b the
// two channels' ramps, the recombined bin W = D_a R_a + i D_b R_b of the pair
// row (D_a = (Z + conj Zm)/2, D_b = (Z - conj Zm)/2i) is
//     W = E (Z cos d - i conj(Zm) sin d),   E = e^{-i (alpha + beta)/2},
//                                           d = (alpha - beta)/2,
// because (R_a + R_b)/2 = E cos d and (R_a - R_b)/2 = -i E sin d.  E and
// D = e^{-i d} come from the half words h = w >> 1 (h_a + h_b and h_a - h_b):
// any h with 2h = w mod 2^64 gives the same W (a dropped top bit flips E and
// D together by (-1)^k'), so no extra host data is needed.  Per bin that is
// two complex products for E and D (base(kb0) x table[q], as before) plus
// four products and one complex product for W: 16 VALU instead of 22.
// Per-pair factors: bin kb0 + q N/RFL has phase offset q (N/RFL) h - [2q >=
// RFL] N h relative to kb0; tabulated once per run in double precision,
// tab[pair][q] = {E factor, D factor}.
template <int RFL>
__global__ void k_pair_tab(const uint64_t *ramp, int64_t N, int nchan, int poff, int npairs, cf *tab) {
    const int pr = blockIdx.x, q = threadIdx.x;
    if (pr >= npairs || q >= RFL) return;
    const int ra = max(2 * pr - poff, 0), rb = min(2 * pr + 1 - poff, nchan - 1);
    const uint64_t ha = (uint64_t)ramp[ra] >> 1, hb = (uint64_t)ramp[rb] >> 1;
    const uint64_t h2[2] = {ha + hb, ha - hb};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        uint64_t ph = (uint64_t)q * ((uint64_t)(N / RFL) * h2[e]);
        if (2 * q >= RFL) ph -= (uint64_t)N * h2[e];
        const double rev = (double)(int64_t)ph * 5.421010862427522e-20;   // 2^-64
        double sn, cs;
        sincospi(2.0 * rev, &sn, &cs);
        tab[((int64_t)pr * RFL + q) * 2 + e] = make_float2((float)cs, (float)(-sn));
    }
}

template <int N2, int T, typename FWD, typename INV>
struct PairRows;

template <int N2, int T, int... F, int... I>
struct PairRows<N2, T, RList<F...>, RList<I...>> {
    // row pitch N2 + 16 (a multiple of 16 complex: the byte-address XOR
    // exchanges, Fft::XB; the rows' bank offset is irrelevant here -- every
    // wave works on one row per instruction)
    using FF = Fft<N2, 2, T, false, 16>;
    using LD = typename FF::LD;
    static constexpr int E = FF::E;
    static constexpr int RF0 = FF::template first<F...>();
    static constexpr int RFL = FF::template last_of<F...>();
    static constexpr int RIL = FF::template last_of<I...>();
    static_assert(RIL == RF0, "inverse plan must be the reversed forward plan");
    static constexpr int LR = N2 / RF0;
    static constexpr int LRL = N2 / RFL;
    // minimum waves per SIMD the kernel is compiled for (VGPR budget 512 /
    // waves): two workgroups per CU when two rows fit twice in LDS
    static constexpr int kMinWaves = (T <= 512) ? 2 * T / 256 : 4;
    // byte offset of (row, n2) in a pair spill, and the offset step of the
    // q-th first-stage input (n2 + q LR)
    static constexpr uint32_t kQS = 8u * (uint32_t)LR;
    __device__ static __forceinline__ uint32_t spill_off(uint32_t RP, int row, int n2) {
        return ((uint32_t)row * RP + (uint32_t)n2) * 8u;
    }

    // MASK = false: data pair of channels (2pr - poff, 2pr + 1 - poff).
    // MASK = true : node pair (2pr, 2pr + 1) of the mask table build -- the
    //               once-per-run mask spectrum times each node's ramp.
    // HT: a per-bin transfer function H (PssPipeline.htab: the baseband
    // coherent dispersion, ism.py:76-98) instead of the delay ramps -- one H
    // for every channel, so the packed pair's bins are simply H_ext(k) Z(k)
    // (H_ext(N - k) = conj H(k); DC and Nyquist x Re H, the irfft rule).
    template <bool MASK, bool TAIL = false, bool HT = false>
    __device__ static void pass(const KP &k) {
        __shared__ __align__(128) cf lds[2 * LD::RS];
        __shared__ cf tw16[kTw16Size];
        const int tid = threadIdx.x;
        tw16_fill(tw16, tid, T);     // first read after the first stage's barrier
        const int pr = blockIdx.x;                 // channel pair
        const int j = blockIdx.y;                  // row pair {j, N1-j}; {0, N1/2}
        const int N1 = (int)k.N1;
        const int rowA = j, rowB = (j == 0) ? N1 / 2 : N1 - j;
        const int off = MASK ? 0 : k.poff;
        const int ra = max(2 * pr - off, 0), rb = min(2 * pr + 1 - off, k.p.nchan - 1);
        const bool data = !MASK;
        const bool mask = MASK;
        const uint64_t rwa = HT ? 0ull : (uint64_t)k.p.ramp[ra], rwb = HT ? 0ull : (uint64_t)k.p.ramp[rb];
        // uniform 64-bit phase offsets of bin kb0 + q N/RFL relative to kb0 (SALU)
        const uint64_t sta = (uint64_t)(k.N / RFL) * rwa, stb = (uint64_t)(k.N / RFL) * rwb;
        const uint64_t nwa = (uint64_t)k.N * rwa, nwb = (uint64_t)k.N * rwb;
        cf v[E];
        const uint32_t pbytes = (uint32_t)(pstride(k) * 8);
        const uint32_t RP = (uint32_t)rpitch(k);
        if (data) {
            const Buf Y(k.Yd + (int64_t)pr * pstride(k), pbytes);
#pragma unroll
            for (int ib = 0; ib < E / RF0; ++ib) {
                const int jj0 = tid + ib * T, b = jj0 / LR, jj = jj0 - b * LR;
                const uint32_t off = spill_off(RP, b ? rowB : rowA, jj);
#pragma unroll
                for (int q = 0; q < RF0; ++q) v[ib * RF0 + q] = Y.ld2(off, q * kQS);
            }
            FF::template run_tw<false, 1, F...>(v, lds, tid, tw16);
            if constexpr (HT) {
                // bin kb0 + q N/RFL of butterfly ib (no mirror bins needed)
                const cf *H = reinterpret_cast<const cf *>(k.p.htab);
#pragma unroll
                for (int ib = 0; ib < E / RFL; ++ib) {
                    const int jg = tid + ib * T, b = jg / LRL, jj = jg - b * LRL;
                    const int64_t kb0 = (b ? rowB : rowA) + (int64_t)N1 * jj;
#pragma unroll
                    for (int q = 0; q < RFL; ++q) {
                        const int64_t kb = kb0 + (int64_t)q * (k.N / RFL);
                        const bool upper = 2 * kb > k.N;
                        const cf h = H[upper ? k.N - kb : kb];
                        cf &z = v[ib * RFL + q];
                        if (kb == 0 || 2 * kb == k.N) z = make_float2(z.x * h.x, z.y * h.x);
                        else z = cmul(z, make_float2(h.x, upper ? -h.y : h.y));
                    }
                }
            } else {
            FF::template store<RFL>(v, lds, tid);
            __syncthreads();
            // pair ramp factors (k_pair_tab): {E, D} per q, wave-uniform
            const cf *ptab = k.rtab + (int64_t)pr * (2 * RFL);
            const uint64_t hsum = (rwa >> 1) + (rwb >> 1), hdif = (rwa >> 1) - (rwb >> 1);
            // RFL = 16 (the C3 4096-point rows): the bins of a butterfly as one
            // straight-line body under a scalar branch (the form below measured
            // neutral at C3 and 0.8 ms slower on C5's 8192-point rows, RFL = 8,
            // profiles/r03/s6: those keep the per-bin form)
            if constexpr (RFL == 16) {
#pragma unroll
            for (int ib = 0; ib < E / RFL; ++ib) {
                const int jg = tid + ib * T;
                // row side b is wave-uniform when LRL is a multiple of the
                // wave: say so, so the mirror-read choice below is a scalar branch
                const int b = (LRL % 64 == 0) ? __builtin_amdgcn_readfirstlane(jg / LRL) : jg / LRL;
                const int jj = jg - b * LRL;
                const int row = b ? rowB : rowA;
                const int64_t kb0 = row + (int64_t)N1 * jj;
                const cf bE = expi_rev(-fix_to_rev((uint64_t)kb0 * hsum));
                const cf bD = expi_rev(-fix_to_rev((uint64_t)kb0 * hdif));
                const bool dc = (kb0 == 0);                      // one lane of one wave per launch
                // bin q of this butterfly from Z = v[i] and its mirror Zm:
                // W = D_a R_a + i D_b R_b; DC (q = 0) and Nyquist (q = RFL/2)
                // of kb0 = 0 by select (no per-bin branch: the body stays
                // straight-line, so the mirror reads of several bins are in
                // flight together)
                auto bin = [&](int q, cf Zm) {
                    const int i = ib * RFL + q;
                    const cf Z = v[i];
                    // 2 D_a and 2 D_b (DC / Nyquist and the tail extension)
                    const cf Sa = make_float2(Z.x + Zm.x, Z.y - Zm.y);
                    const cf Sb = make_float2(Z.y + Zm.y, Zm.x - Z.x);
                    cf W;
                    {
                        const cf Ef = cmul(bE, ptab[2 * q]), Df = cmul(bD, ptab[2 * q + 1]);
                        if constexpr (TAIL) {
                            // per-channel transfer functions: R_a = E D, R_b = E conj(D)
                            const cf w = bin_phasor(kb0 + (int64_t)q * (k.N / RFL), k.N);
                            const cf ra_ = cmul(make_float2(0.5f * Ef.x, 0.5f * Ef.y), cmul(Df, tail_factor(k.p.tail_a[ra], w)));
                            const cf rb_ = cmul(make_float2(0.5f * Ef.x, 0.5f * Ef.y), cmul_conj(tail_factor(k.p.tail_a[rb], w), Df));
                            const cf A = cmul(Sa, ra_);
                            const cf Bv = cmul(Sb, rb_);
                            W = make_float2(A.x - Bv.y, A.y + Bv.x);
                        } else {
                            // W = E (Z cos d - i conj(Zm) sin d), D = cos d - i sin d
                            const float c = Df.x, s = -Df.y;
                            const cf in = make_float2(fmaf(Z.x, c, -(Zm.y * s)), fmaf(Z.y, c, -(Zm.x * s)));
                            W = cmul(Ef, in);
                        }
                        if (2 * q == RFL) {                         // Nyquist bin (compile-time q)
                            float fa = k.p.nyq_re[ra], fb = k.p.nyq_re[rb];
                            if constexpr (TAIL) {                   // H(N/2) = (1-a)/(1+a)
                                const float ta = k.p.tail_a[ra], tb = k.p.tail_a[rb];
                                fa *= (1.0f - ta) / (1.0f + ta);
                                fb *= (1.0f - tb) / (1.0f + tb);
                            }
                            const cf Wn = make_float2((0.5f * Sa.x) * fa, (0.5f * Sb.x) * fb);
                            W = dc ? Wn : W;
                        } else if (q == 0) {                        // DC (H = 1)
                            const cf Da = make_float2(0.5f * Sa.x, 0.5f * Sa.y), Db = make_float2(0.5f * Sb.x, 0.5f * Sb.y);
                            const cf Wd = make_float2(Da.x - Db.y, Da.y + Db.x);
                            W = dc ? Wd : W;
                        }
                    }
                    v[i] = W;
                };
                // mirror bins k2m = N2 - 1 - k2 = P0 - q LRL (all but row 0 of
                // the {0, N1/2} pair, whose bin 0 pairs with itself): with
                // LRL % 256 == 0 the swizzle XOR is the same for every q, so
                // the reads are one byte base minus immediate offsets.  The
                // choice is one scalar branch around the whole bin loop.
                constexpr bool kMirXB = FF::XB && (LRL % 256 == 0);
                const bool affine = !(j == 0 && row == 0);       // wave-uniform
                if (kMirXB && affine) {
                    const uint32_t mbase = lds_byte(lds) + 8u * (uint32_t)LD::at(j == 0 ? b : 1 - b, N2 - 1 - jj);
#pragma unroll
                    for (int q = 0; q < RFL; ++q) bin(q, lds_ld(mbase - 8u * (uint32_t)(q * LRL)));
                } else {
#pragma unroll
                    for (int q = 0; q < RFL; ++q) {
                        const int k2 = jj + q * LRL;
                        int bm, k2m;
                        if (j == 0) { bm = b; k2m = (row == 0) ? (((N2 & (N2 - 1)) == 0) ? ((N2 - k2) & (N2 - 1)) : (k2 ? N2 - k2 : 0)) : (N2 - 1 - k2); }
                        else        { bm = 1 - b; k2m = N2 - 1 - k2; }
                        bin(q, lds[LD::at(bm, k2m)]);
                    }
                }
            }
            } else {
#pragma unroll
            for (int ib = 0; ib < E / RFL; ++ib) {
                const int jg = tid + ib * T, b = jg / LRL, jj = jg - b * LRL;
                const int row = b ? rowB : rowA;
                const int64_t kb0 = row + (int64_t)N1 * jj;
                const cf bE = expi_rev(-fix_to_rev((uint64_t)kb0 * hsum));
                const cf bD = expi_rev(-fix_to_rev((uint64_t)kb0 * hdif));
                // mirror bins k2m = N2 - 1 - k2 = P0 - q LRL (all but row 0 of
                // the {0, N1/2} pair, whose bin 0 pairs with itself): with
                // LRL % 256 == 0 the swizzle XOR is the same for every q, so
                // the reads are one byte base minus immediate offsets
                constexpr bool kMirXB = FF::XB && (LRL % 256 == 0);
                const bool affine = !(j == 0 && row == 0);       // wave-uniform
                uint32_t mbase = 0;
                if constexpr (kMirXB) mbase = lds_byte(lds) + 8u * (uint32_t)LD::at(j == 0 ? b : 1 - b, N2 - 1 - jj);
#pragma unroll
                for (int q = 0; q < RFL; ++q) {
                    const int i = ib * RFL + q, k2 = jj + q * LRL;
                    cf Zm;
                    if (kMirXB && affine) {
                        Zm = lds_ld(mbase - 8u * (uint32_t)(q * LRL));
                    } else {
                        int bm, k2m;
                        if (j == 0) { bm = b; k2m = (row == 0) ? (((N2 & (N2 - 1)) == 0) ? ((N2 - k2) & (N2 - 1)) : (k2 ? N2 - k2 : 0)) : (N2 - 1 - k2); }
                        else        { bm = 1 - b; k2m = N2 - 1 - k2; }
                        Zm = lds[LD::at(bm, k2m)];
                    }
                    const cf Z = v[i];
                    // 2 D_a and 2 D_b (DC / Nyquist and the tail extension)
                    const cf Sa = make_float2(Z.x + Zm.x, Z.y - Zm.y);
                    const cf Sb = make_float2(Z.y + Zm.y, Zm.x - Z.x);
                    if (kb0 == 0 && 2 * q == RFL) {                 // Nyquist bin
                        float fa = k.p.nyq_re[ra], fb = k.p.nyq_re[rb];
                        if constexpr (TAIL) {                       // H(N/2) = (1-a)/(1+a)
                            const float ta = k.p.tail_a[ra], tb = k.p.tail_a[rb];
                            fa *= (1.0f - ta) / (1.0f + ta);
                            fb *= (1.0f - tb) / (1.0f + tb);
                        }
                        v[i] = make_float2((0.5f * Sa.x) * fa, (0.5f * Sb.x) * fb);
                    } else if (kb0 == 0 && q == 0) {                // DC (H = 1)
                        const cf Da = make_float2(0.5f * Sa.x, 0.5f * Sa.y), Db = make_float2(0.5f * Sb.x, 0.5f * Sb.y);
                        v[i] = make_float2(Da.x - Db.y, Da.y + Db.x);
                    } else {
                        const cf Ef = cmul(bE, ptab[2 * q]), Df = cmul(bD, ptab[2 * q + 1]);
                        if constexpr (TAIL) {
                            // per-channel transfer functions: R_a = E D, R_b = E conj(D)
                            const cf w = bin_phasor(kb0 + (int64_t)q * (k.N / RFL), k.N);
                            const cf ra_ = cmul(make_float2(0.5f * Ef.x, 0.5f * Ef.y), cmul(Df, tail_factor(k.p.tail_a[ra], w)));
                            const cf rb_ = cmul(make_float2(0.5f * Ef.x, 0.5f * Ef.y), cmul_conj(tail_factor(k.p.tail_a[rb], w), Df));
                            const cf A = cmul(Sa, ra_);
                            const cf Bv = cmul(Sb, rb_);
                            v[i] = make_float2(A.x - Bv.y, A.y + Bv.x);
                        } else {
                            // W = E (Z cos d - i conj(Zm) sin d), D = cos d - i sin d
                            const float c = Df.x, s = -Df.y;
                            const cf in = make_float2(fmaf(Z.x, c, -(Zm.y * s)), fmaf(Z.y, c, -(Zm.x * s)));
                            v[i] = cmul(Ef, in);
                        }
                    }
                }
            }
            }
            }   // (HT)
            __syncthreads();
            FF::template run_tw<true, 1, I...>(v, lds, tid, tw16);
#pragma unroll
            for (int ib = 0; ib < E / RF0; ++ib) {
                const int jj0 = tid + ib * T, b = jj0 / LR, jj = jj0 - b * LR;
                const uint32_t off = spill_off(RP, b ? rowB : rowA, jj);
#pragma unroll
                for (int q = 0; q < RF0; ++q) Y.st2(v[ib * RF0 + q], off, q * kQS);
            }
        }
        if (mask) {
            const Buf V(k.Ym + (int64_t)pr * pstride(k), pbytes);
            const Buf Ms(k.Mspec, (uint32_t)(k.N * 8));      // [N1][N2], no spill pad
#pragma unroll
            for (int ib = 0; ib < E / RFL; ++ib) {
                const int jg = tid + ib * T, b = jg / LRL, jj = jg - b * LRL;
                const int row = b ? rowB : rowA;
                const int64_t kb0 = row + (int64_t)N1 * jj;
                const uint64_t p0a = (uint64_t)kb0 * rwa, p0b = (uint64_t)kb0 * rwb;
                const uint32_t moff = (uint32_t)(row * N2 + jj) * 8u;
#pragma unroll
                for (int q = 0; q < RFL; ++q) {
                    const int i = ib * RFL + q;
                    const cf M = Ms.ld2(moff, q * LRL * 8);
                    if (kb0 == 0 && 2 * q == RFL) {                 // Nyquist bin
                        v[i] = make_float2(M.x * k.p.nyq_im[ra], M.x * k.p.nyq_im[rb]);
                    } else if (kb0 == 0 && q == 0) {                // DC: M (1 + i)
                        v[i] = make_float2(M.x - M.y, M.y + M.x);
                    } else {                                        // M (R_a + i R_b)
                        const cf Ra = ramp_q<RFL>(p0a, sta, nwa, q), Rb = ramp_q<RFL>(p0b, stb, nwb, q);
                        v[i] = cmul(M, make_float2(Ra.x - Rb.y, Ra.y + Rb.x));
                    }
                }
            }
            __syncthreads();
            FF::template run_tw<true, 1, I...>(v, lds, tid, tw16);
#pragma unroll
            for (int ib = 0; ib < E / RF0; ++ib) {
                const int jj0 = tid + ib * T, b = jj0 / LR, jj = jj0 - b * LR;
                const uint32_t off = spill_off(RP, b ? rowB : rowA, jj);
#pragma unroll
                for (int q = 0; q < RF0; ++q) V.st2(v[ib * RF0 + q], off, q * kQS);
            }
        }
    }
};

template <typename R, int T, bool TAIL = false, bool HT = false>
__global__ __launch_bounds__(T, R::kMinWaves) void k_pair_row(KP k) { R::template pass<false, TAIL, HT>(k); }
template <typename R, int T>
__global__ __launch_bounds__(T) void k_node_row(KP k) { R::template pass<true>(k); }

// Row pass of a data pair with the two rows of a row pair in registers and
// ONE row in LDS (the 8192-point rows of C5's 2048 x 8192
// split): PairRows holds both rows in LDS (2 x 65.7 KB, one workgroup per
// CU, so every barrier stalls the CU); here each exchange moves one row
// through a 65.7-KB buffer and two workgroups share a CU.  Same stages and
// ramp arithmetic as PairRows::pass<false> (no tail extension).  After the
// forward transforms a thread holds row A's bins k2 = jj + q LRL and row
// B's at the mirrors N2-1-k2 (row B's thread relabelling below); it forms
// W_A(k2) and W_B(N2-1-k2) from the same pair of registers.  Row pair {0,
// N1/2} (each row its own mirror, DC and Nyquist in row 0) takes the
// per-row form through LDS.
template <int N2, int T, typename FWD, typename INV>
struct PairRowsSeq;

// a value the compiler cannot see through (no CSE across uses)
__device__ __forceinline__ int opaque(int x) {
    asm volatile("" : "+v"(x));
    return x;
}

template <int N2, int T, int... F, int... I>
struct PairRowsSeq<N2, T, RList<F...>, RList<I...>> {
    using FF = Fft<N2, 1, T, false, 16>;
    using LD = typename FF::LD;
    using PRW = PairRows<N2, T, RList<F...>, RList<I...>>;   // spill addressing
    static constexpr int E = FF::E;                           // values per thread of ONE row
    static constexpr int RF0 = FF::template first<F...>();
    static constexpr int RFL = FF::template last_of<F...>();
    static constexpr int LR = N2 / RF0;
    static constexpr int LRL = N2 / RFL;
    static_assert(FF::template last_of<I...>() == RF0 && FF::template first<I...>() == RFL,
                  "inverse plan must be the reversed forward plan");
    static_assert(E / RF0 * T <= LR && E / RFL * T <= LRL, "one row per thread mapping");

    // W = E (Z cos d - i conj(Zm) sin d) of bin kb0 + q N/RFL (PairRows::pass)
    __device__ static __forceinline__ cf ramp(cf Z, cf Zm, cf bE, cf bD, const cf *ptab, int q) {
        const cf Ef = cmul(bE, ptab[2 * q]), Df = cmul(bD, ptab[2 * q + 1]);
        const float c = Df.x, s = -Df.y;
        return cmul(Ef, make_float2(fmaf(Z.x, c, -(Zm.y * s)), fmaf(Z.y, c, -(Zm.x * s))));
    }

    // SELF: row pair {0, N1/2} (its own launch: a branch between the two
    // forms makes the compiler spill both rows at the branch)
    template <bool SELF>
    __device__ static void pass(const KP &k) {
        __shared__ __align__(128) cf lds[LD::RS];
        __shared__ cf tw16[kTw16Size];
        const int tid = threadIdx.x;
        tw16_fill(tw16, tid, T);
        const int pr = blockIdx.x;
        const int j = SELF ? 0 : (int)blockIdx.y + 1;   // row pair {j, N1-j}; {0, N1/2}
        const int N1 = (int)k.N1;
        const int rowA = j, rowB = (j == 0) ? N1 / 2 : N1 - j;
        const int ra = max(2 * pr - k.poff, 0), rb = min(2 * pr + 1 - k.poff, k.p.nchan - 1);
        const uint64_t rwa = (uint64_t)k.p.ramp[ra], rwb = (uint64_t)k.p.ramp[rb];
        const uint64_t hsum = (rwa >> 1) + (rwb >> 1), hdif = (rwa >> 1) - (rwb >> 1);
        const cf *ptab = k.rtab + (int64_t)pr * (2 * RFL);
        const uint32_t RP = (uint32_t)rpitch(k);
        const Buf Y(k.Yd + (int64_t)pr * pstride(k), (uint32_t)(pstride(k) * 8));
        cf va[E], vb[E];
        // one row's registers live across the other's transform, not two
        // rows' loads in flight (the 128-VGPR budget of 4 waves per SIMD)
        auto load = [&](cf (&v)[E], int row, int b, int t) __attribute__((always_inline)) {
#pragma unroll
            for (int ib = 0; ib < E / RF0; ++ib) {
                const uint32_t o = PRW::spill_off(RP, row, t + ib * T);
#pragma unroll
                for (int q = 0; q < RF0; ++q) v[ib * RF0 + q] = Y.ld2(o, q * PRW::kQS);
            }
        };
        // Row B runs as thread tb = T-1-tid (a relabelling of the threads:
        // every stage and both spill accesses use tb).  With LRL = (E/RFL) T
        // its last forward stage leaves, in register E-1-i, row B's bin
        // N2-1-k2 -- the mirror of row A's bin k2 in register i -- so the
        // ramp pairs registers without an LDS exchange, and W_B is already
        // in thread tb's inverse input mapping.
        const int tb = SELF ? tid : T - 1 - tid;
        // (each transform ends with a barrier after its last LDS read, so
        // the next one may scatter at once)
        // opaque(...) per transform: the four transforms have identical
        // LDS address arithmetic, and without it the compiler keeps one
        // set of addresses live across the kernel (spilled) instead of
        // recomputing them
        load(va, rowA, 0, tid);
        FF::template run_tw<false, 1, F...>(va, lds, opaque(tid), tw16);
        load(vb, rowB, 1, tb);
        FF::template run_tw<false, 1, F...>(vb, lds, opaque(tb), tw16);
        if constexpr (!SELF) {
            static_assert(E / RFL * T == LRL, "mirror registers need LRL = (E/RFL) T");
#pragma unroll
            for (int ib = 0; ib < E / RFL; ++ib) {
                const int jj = tid + ib * T, jm = LRL - 1 - jj;
                const int64_t ka = rowA + (int64_t)N1 * jj, kbm = rowB + (int64_t)N1 * jm;
                const cf aE = expi_rev(-fix_to_rev((uint64_t)ka * hsum));
                const cf aD = expi_rev(-fix_to_rev((uint64_t)ka * hdif));
                const cf bE = expi_rev(-fix_to_rev((uint64_t)kbm * hsum));
                const cf bD = expi_rev(-fix_to_rev((uint64_t)kbm * hdif));
#pragma unroll
                for (int q = 0; q < RFL; ++q) {
                    const int i = ib * RFL + q;
                    const cf Za = va[i], Zb = vb[E - 1 - i];      // A at k2, B at N2-1-k2
                    va[i] = ramp(Za, Zb, aE, aD, ptab, q);
                    vb[E - 1 - i] = ramp(Zb, Za, bE, bD, ptab, RFL - 1 - q);
                }
            }
        } else {
            // rows 0 and N1/2: each its own mirror (row 0: bin 0 with itself)
            auto self = [&](cf (&v)[E], int row) __attribute__((always_inline)) {
                FF::template store<RFL>(v, lds, opaque(tid));
                __syncthreads();
#pragma unroll
                for (int ib = 0; ib < E / RFL; ++ib) {
                    const int jj = tid + ib * T;
                    const int64_t kb0 = row + (int64_t)N1 * jj;
                    const cf bE = expi_rev(-fix_to_rev((uint64_t)kb0 * hsum));
                    const cf bD = expi_rev(-fix_to_rev((uint64_t)kb0 * hdif));
#pragma unroll
                    for (int q = 0; q < RFL; ++q) {
                        const int i = ib * RFL + q, k2 = jj + q * LRL;
                        const int k2m = (row == 0) ? (((N2 & (N2 - 1)) == 0) ? ((N2 - k2) & (N2 - 1)) : (k2 ? N2 - k2 : 0)) : (N2 - 1 - k2);
                        const cf Z = v[i], Zm = lds[LD::at(0, k2m)];
                        const cf Sa = make_float2(Z.x + Zm.x, Z.y - Zm.y);
                        const cf Sb = make_float2(Z.y + Zm.y, Zm.x - Z.x);
                        if (kb0 == 0 && 2 * q == RFL) {          // Nyquist bin
                            v[i] = make_float2((0.5f * Sa.x) * k.p.nyq_re[ra], (0.5f * Sb.x) * k.p.nyq_re[rb]);
                        } else if (kb0 == 0 && q == 0) {         // DC (H = 1)
                            const cf Da = make_float2(0.5f * Sa.x, 0.5f * Sa.y), Db = make_float2(0.5f * Sb.x, 0.5f * Sb.y);
                            v[i] = make_float2(Da.x - Db.y, Da.y + Db.x);
                        } else {
                            v[i] = ramp(Z, Zm, bE, bD, ptab, q);
                        }
                    }
                }
                __syncthreads();
            };
            self(va, rowA);
            self(vb, rowB);
        }
        FF::template run_tw<true, 1, I...>(va, lds, opaque(tid), tw16);
#pragma unroll
        for (int ib = 0; ib < E / RF0; ++ib) {
            const int jj = tid + ib * T;
            const uint32_t oa = PRW::spill_off(RP, rowA, jj);
#pragma unroll
            for (int q = 0; q < RF0; ++q) Y.st2(va[ib * RF0 + q], oa, q * PRW::kQS);
        }
        FF::template run_tw<true, 1, I...>(vb, lds, opaque(tb), tw16);
#pragma unroll
        for (int ib = 0; ib < E / RF0; ++ib) {
            const int jj = tb + ib * T;
            const uint32_t ob = PRW::spill_off(RP, rowB, jj);
#pragma unroll
            for (int q = 0; q < RF0; ++q) Y.st2(vb[ib * RF0 + q], ob, q * PRW::kQS);
        }
    }
};

template <typename R, int T, bool SELF>
__global__ __launch_bounds__(T, SELF ? 1 : 4) void k_pair_row_seq(KP k) { R::template pass<SELF>(k); }


// XRS: extra row pitch of the LDS column block (Lds), chosen per kernel for
// its transposing accesses (xrs_read and ColEngine below).
template <int N1, int B, int T, typename FWD, typename INV, int XRS = 1>
struct PairCols;

template <int N1, int B, int T, int... F, int... I, int XRS>
struct PairCols<N1, B, T, RList<F...>, RList<I...>, XRS> {
    using LdsC = Lds<N1, XRS>;
    using FF = Fft<N1, B, T, false, XRS>;
    static constexpr int E = FF::E;
    // One wave per column (T = 64 B, N1/64 values per lane): the column FFTs
    // are wave-local (Fft<..., WAVE>: no workgroup barrier between stages);
    // only the transposes between sample-major items and columns need one.
    using FW = Fft<(N1 % 64 == 0 ? N1 : 64), 1, 64, true, XRS>;   // same row layout as LdsC (placeholder when N1 % 64 != 0)
    static constexpr bool kWaveCols = (T == 64 * B) && (N1 % 64 == 0) && (N1 / 64 == E);
    // pass A: four-step twiddle folded into the column FFT's last stage
    static constexpr bool kMergeTw = sizeof...(F) >= 2;
    static constexpr int RF0 = FF::template first<F...>();
    static constexpr int RFL = FF::template last_of<F...>();
    static constexpr int RI0 = FF::template first<I...>();
    static constexpr int RIL = FF::template last_of<I...>();
    static constexpr int ITEMS = N1 * B / 4 / T;
    // the unrolled fast kernels need a whole number of 4-sample items per
    // thread (N1 = 2^m); the generic ones loop (any N1, e.g. 30 = 2 * 3 * 5)
    static constexpr bool kItemsExact = ITEMS * 4 * T == N1 * B;
    // Mixed-radix columns (N1 not a power of two, one column per thread, B
    // == T): the column DFTs run in registers (RegDft: compile-time twiddles,
    // no LDS exchange), the spill is written / read one column per lane
    // (consecutive lanes = consecutive columns: coalesced rows)
    static constexpr bool kRegCols = (B == T) && ((N1 & (N1 - 1)) != 0);
    static constexpr int kFoldWaves = N1 <= 30 ? 4 : 2;      // min waves per SIMD of the fold kernels
    // passC_fold's lane-private LDS (N1 x 8 B per lane) caps its waves per
    // SIMD at (160 KB / (N1 x 8 B x B)) x B / 256
    static constexpr int kFoldWavesC = (160 * 1024 / (N1 * 8 * B)) * B / 256 < 1 ? 1
                                     : ((160 * 1024 / (N1 * 8 * B)) * B / 256 > 4 ? 4 : (160 * 1024 / (N1 * 8 * B)) * B / 256);
    static_assert(B % 4 == 0, "4-sample items");

    // Pass A's 4-sample item it of a column block: row n1, first column b4.
    // Lanes = consecutive rows n1 (of one 4-column group where N1 % 64 == 0):
    // the transposed LDS writes are conflict-free.
    __device__ static __forceinline__ void item_of(int it, int &n1, int &b4) {
        if constexpr (N1 % 64 == 0) {
            n1 = it % N1;
            b4 = (it / N1) * 4;
        } else {
            n1 = it / (B / 4);
            b4 = (it - n1 * (B / 4)) * 4;
        }
    }

    // The shared profile (prof_rows == 1: one PCHIP row for every channel,
    // e.g. C3's GaussProfile) is a function of the sample alone, so it is
    // evaluated once per run instead of once per pair: entry cbx (N1 B / 4) +
    // it holds samples n .. n + 3 of item it of column block cbx, so each
    // pass-A workgroup reads one contiguous 4 N1 B-byte block (a wave 1 KB per
    // item) in place of a phase walk, an LDS gather and a cubic per sample.
    // The same integer walk and the same fused cubic as the per-pair form:
    // bitwise its values.
    __device__ static void prof_cols(const KP &k, float4 *out) {
        const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (e >= k.N / 4) return;
        constexpr int IPB = N1 * B / 4;                 // items per column block
        const int cbx = (int)(e / IPB), it = (int)(e - (int64_t)cbx * IPB);
        int n1, b4;
        item_of(it, n1, b4);
        const PssPipeline &p = k.p;
        const uint32_t n = (uint32_t)(n1 * (int)k.N2) + (uint32_t)(cbx * B) + (uint32_t)b4;   // N < 2^24
        uint32_t dlo;
        uint64_t dhi;
        phase_delta(p, dlo, dhi);
        const float4 *prof = reinterpret_cast<const float4 *>(p.prof);
        PhaseWalk w;
        w.start(p, n);
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t iv;
            float u;
            if (i) w.step(dlo, dhi, p.knot_m);
            w.get_full(iv, u);
            const float4 A = prof[iv];
            v[i] = fmaf(fmaf(fmaf(A.x, u, A.y), u, A.z), u, A.w);
        }
        out[e] = make_float4(v[0], v[1], v[2], v[3]);
    }

    // A: generate channels a, b into z = d_a + i d_b; column FFTs; twiddle; spill.
    // FAST (host-selected): search-mode source with Philox chi2(1) draws, no
    // injected draws, no undelayed null -- the same values as source4.
    template <bool FAST, bool SHARED = false>
    __device__ static void passA(const KP &k) {
        __shared__ __align__(128) cf lds[B * LdsC::RS];   // (128-B aligned: the FFT's byte-address exchanges)
        __shared__ cf tw16[kTw16Size];
        const int tid = threadIdx.x;
        tw16_fill(tw16, tid, T);     // read after the generate loop's barrier
        int cbx, pr;
        xcd_block(cbx, pr);
        const int ra = 2 * pr - k.poff, rb = ra + 1;
        const bool hasa = ra >= 0, hasb = rb < k.p.nchan;
        const int64_t n20 = (int64_t)cbx * B;
        const int64_t N2 = k.N2;
        const PssPipeline &p = k.p;
        const uint32_t ca = (uint32_t)(p.chan0 + ra), cb = ca + 1u;
        const int pra = (p.prof_rows == 1) ? 0 : (int)ca - p.prof_row0, prb = (p.prof_rows == 1) ? 0 : (int)cb - p.prof_row0;
        const Rng g(p.seed, p.call_gen, P_PULSE);
        static_assert(!FAST || kItemsExact, "fast pass A: whole items per thread");
        if constexpr (FAST && SHARED) {
            // (host-selected: prof_rows == 1, e.g. C3's GaussProfile)
            // the profile from the per-run sample table (prof_cols): loads
            // issued first, under the Philox draws
            const float dna = hasa ? p.draw_norm : 0.f, dnb = hasb ? p.draw_norm : 0.f;
            const float4 *pc = k.pcol + (int64_t)cbx * (N1 * B / 4);
            float4 P[ITEMS];
#pragma unroll
            for (int t = 0; t < ITEMS; ++t) P[t] = pc[tid + t * T];
#pragma unroll
            for (int t = 0; t < ITEMS; ++t) {
                const int it = tid + t * T;
                int n1, b4;
                item_of(it, n1, b4);
                const uint32_t n = (uint32_t)(n1 * (int)N2) + (uint32_t)n20 + (uint32_t)b4;   // N < 2^24
                const float4 qa = chi2_1x4(g.bits(n >> 2, ca, 0u), dna);
                const float4 qb = chi2_1x4(g.bits(n >> 2, cb, 0u), dnb);
                const float pv[4] = {P[t].x, P[t].y, P[t].z, P[t].w};
                const float va[4] = {qa.x, qa.y, qa.z, qa.w}, vb[4] = {qb.x, qb.y, qb.z, qb.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) lds[LdsC::at(b4 + i, n1)] = make_float2(pv[i] * va[i], pv[i] * vb[i]);
            }
        } else if constexpr (FAST) {
            // The pair's two PCHIP rows are staged in LDS (host guarantees
            // nint <= kFastNint), the items are unrolled and branch-free, so
            // the table reads of an item issue together instead of one
            // exposed global-load latency per sample.
            __shared__ float4 ptab[2][kFastNint];
            const int nint = p.nint;
            const int last = p.prof_rows - 1;
            const int rowa = min(max(pra, 0), last), rowb = min(max(prb, 0), last);
            const float4 *prof = reinterpret_cast<const float4 *>(p.prof);
            for (int i = tid; i < nint; i += T) {
                ptab[0][i] = prof[(int64_t)rowa * nint + i];
                ptab[1][i] = prof[(int64_t)rowb * nint + i];
            }
            __syncthreads();
            // draw_norm, or 0 for a pair's missing channel (shard / band
            // edges): the multiply the sample needs anyway zeroes it, no select
            const float dna = hasa ? p.draw_norm : 0.f, dnb = hasb ? p.draw_norm : 0.f;
            // item = 4 consecutive samples n .. n + 3 of row n1 (Philox block
            // n >> 2, at every N), phases by a unit walk
            uint32_t dlo;
            uint64_t dhi;
            phase_delta(p, dlo, dhi);
            const uint32_t M = p.knot_m;
#pragma unroll
            for (int t = 0; t < ITEMS; ++t) {
                // lanes = consecutive rows n1 (of one 4-column group where
                // N1 % 64 == 0): the transposed LDS writes below are
                // conflict-free (this loop touches no global memory, so its
                // item order is free)
                const int it = tid + t * T;
                int n1, b4;
                if constexpr (N1 % 64 == 0) {
                    n1 = it % N1;
                    b4 = (it / N1) * 4;
                } else {
                    n1 = it / (B / 4);
                    b4 = (it - n1 * (B / 4)) * 4;
                }
                const uint32_t n = (uint32_t)(n1 * (int)N2) + (uint32_t)n20 + (uint32_t)b4;   // N < 2^24
                // draws scaled by draw_norm (0 for a pair's missing channel) in the sampler
                const float4 qa = chi2_1x4(g.bits(n >> 2, ca, 0u), dna);
                const float4 qb = chi2_1x4(g.bits(n >> 2, cb, 0u), dnb);
                const float va[4] = {qa.x, qa.y, qa.z, qa.w}, vb[4] = {qb.x, qb.y, qb.z, qb.w};
                PhaseWalk w;
                w.start(p, n);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    uint32_t iv;
                    float u;
                    if (i) w.step(dlo, dhi, M);
                    w.get_full(iv, u);       // fast_source(): nint == knot_m
                    const float4 A = ptab[0][iv];
                    const float pa = fmaf(fmaf(fmaf(A.x, u, A.y), u, A.z), u, A.w);
                    const float4 Bc = ptab[1][iv];
                    const float pb = fmaf(fmaf(fmaf(Bc.x, u, Bc.y), u, Bc.z), u, Bc.w);
                    lds[LdsC::at(b4 + i, n1)] = make_float2(pa * va[i], pb * vb[i]);
                }
            }
        } else
        for (int it = tid; it < N1 * B / 4; it += T) {
            const int n1 = it / (B / 4);
            const int b4 = (it - n1 * (B / 4)) * 4;
            const int64_t n = n1 * N2 + n20 + b4;
            float xa[4], xb[4], dum[4];
            if (hasa) source4(k, ra, n, 4, xa, dum, true, false);
            else { xa[0] = xa[1] = xa[2] = xa[3] = 0.f; }
            if (hasb) source4(k, rb, n, 4, xb, dum, true, false);
            else { xb[0] = xb[1] = xb[2] = xb[3] = 0.f; }
#pragma unroll
            for (int i = 0; i < 4; ++i) lds[LdsC::at(b4 + i, n1)] = make_float2(xa[i], xb[i]);
        }
        __syncthreads();
        if constexpr (kRegCols) {
            cf x[N1];
#pragma unroll
            for (int n1 = 0; n1 < N1; ++n1) x[n1] = lds[LdsC::at(tid, n1)];
            reg_spill(k, x, pr, n20 + tid);
            return;
        }
        cf v[E];
        const float invN = k.invN;
        if constexpr (kWaveCols) {
            // wave w transforms column w in its own LDS row
            const int wv = tid >> 6, lane = tid & 63;
            cf *wl = lds + wv * LdsC::RS;
            FW::template load<RF0>(v, wl, lane);
            stage_sync<true>();
            if constexpr (kMergeTw) {
                // Last stage (radix RFL at Ns = N1/RFL) with the four-step
                // twiddle folded in.  Output m of butterfly jj is k1 = jj +
                // Ns m, and W_N^{n2 k1} = W_N^{n2 jj} W_N^{n2 Ns m}: the first
                // factor is common to the butterfly, so it joins the stage's
                // input twiddles W_N1^{jj q} (one phase per input,
                // W_N^{jj (n2 + N2 q)}), the second is wave-uniform (one
                // product per output).  Phases in exact 32-bit fixed point.
                FW::template run_head_tw<false, 1, F...>(v, wl, lane, tw16);
                constexpr int NsL = N1 / RFL;
                constexpr int LG1 = __builtin_ctz((unsigned)N1);
                const int LGN = __builtin_ctzll((unsigned long long)k.N);        // N = 2^LGN here
                const uint32_t A = (uint32_t)(n20 + wv) << (32 - LGN);           // n2 / N (2^-32 rev)
                cf U[RFL];
#pragma unroll
                for (int m = 1; m < RFL; ++m) U[m] = expi_rev(-fix32_to_rev(A * (uint32_t)(NsL * m)));
#pragma unroll
                for (int ib = 0; ib < E / RFL; ++ib) {
                    const uint32_t jj = (uint32_t)(lane + 64 * ib);              // < NsL
                    const uint32_t X0 = jj * A, S = jj << (32 - LG1);
                    cf *a = v + ib * RFL;
#pragma unroll
                    for (int q = 0; q < RFL; ++q) a[q] = cmul(a[q], expi_rev(-fix32_to_rev(X0 + (uint32_t)q * S)));
                    dft<RFL, false>(a);
#pragma unroll
                    for (int m = 1; m < RFL; ++m) a[m] = cmul(a[m], U[m]);
                }
            } else {
                FW::template run_tw<false, 1, F...>(v, wl, lane, tw16);
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    int b0, k1;
                    FW::template where<RFL>(i, lane, b0, k1);
                    const uint32_t m = (uint32_t)(n20 + wv) * (uint32_t)k1;
                    float rev = (float)m * invN;
                    if (rev >= 0.5f) rev -= 1.0f;
                    v[i] = cmul(v[i], expi_rev(-rev));
                }
            }
            FW::template store<RFL>(v, wl, lane);
        } else {
            FF::template load<RF0>(v, lds, tid);
            __syncthreads();
            FF::template run_tw<false, 1, F...>(v, lds, tid, tw16);
#pragma unroll
            for (int i = 0; i < E; ++i) {
                int b, k1;
                FF::template where<RFL>(i, tid, b, k1);
                // (n20 + b) k1 < N1 N2 = N <= 2^24: exact in 32-bit and in float
                const uint32_t m = (uint32_t)(n20 + b) * (uint32_t)k1;
                float rev = (float)m * invN;
                if (rev >= 0.5f) rev -= 1.0f;
                v[i] = cmul(v[i], expi_rev(-rev));
            }
            FF::template store<RFL>(v, lds, tid);
        }
        __syncthreads();
        spill_block(k, lds, tid, pr, n20);
    }

    // The spill of a column block from LDS (natural k1 per column row):
    // 16-B stores of 4 columns per row k1, 32 consecutive rows per 32-lane group.
    __device__ static __forceinline__ void spill_block(const KP &k, const cf *lds, int tid, int pr, int64_t n20) {
        cf *Y = k.Yd + (int64_t)pr * pstride(k);
        const int64_t RP = rpitch(k);
        for (int it = tid; it < N1 * B / 4; it += T) {
            int k1, b4;
            if constexpr (B < 32 && N1 % 32 == 0) {
                // 32-lane groups: 32 consecutive rows of one 4-column group
                // (the lanes of a store instruction still cover whole row
                // segments, two lanes 32 apart per 64-B segment)
                const int g = it >> 5;
                b4 = (g % (B / 4)) * 4;
                k1 = (g / (B / 4)) * 32 + (it & 31);
            } else {
                k1 = it / (B / 4);
                b4 = (it - k1 * (B / 4)) * 4;
            }
            cf a0 = lds[LdsC::at(b4 + 0, k1)], a1 = lds[LdsC::at(b4 + 1, k1)];
            cf a2 = lds[LdsC::at(b4 + 2, k1)], a3 = lds[LdsC::at(b4 + 3, k1)];
            PSS_DASSERT((int64_t)k1 * RP + n20 + b4 + 4 <= pstride(k));
            float4 *dst = reinterpret_cast<float4 *>(Y + (int64_t)k1 * RP + n20 + b4);
            dst[0] = make_float4(a0.x, a0.y, a1.x, a1.y);
            dst[1] = make_float4(a2.x, a2.y, a3.x, a3.y);
        }
    }

    // Register columns (kRegCols): forward DFT of this thread's column n2
    // (x[n1] = z(n1 N2 + n2)), four-step twiddle W_N^{n2 k1}, spill row k1
    // at column n2.
    __device__ static __forceinline__ void reg_spill(const KP &k, cf (&x)[N1], int pr, int64_t n2) {
        static_assert(kRegCols, "register columns only");
        RegDft<N1, false>::run(x);
        const Buf Y(k.Yd + (int64_t)pr * pstride(k), (uint32_t)(pstride(k) * 8));
        const uint32_t RP = (uint32_t)rpitch(k);
        const float invN = k.invN;
#pragma unroll
        for (int k1 = 0; k1 < N1; ++k1) {
            // n2 k1 < N (exact in 32-bit and in float)
            float rev = (float)((uint32_t)n2 * (uint32_t)k1) * invN;
            if (rev >= 0.5f) rev -= 1.0f;
            const cf w = k1 ? cmul(x[k1], expi_rev(-rev)) : x[k1];
            Y.st2(w, ((uint32_t)k1 * RP + (uint32_t)n2) * 8u, 0u);
        }
    }
    // ... and back: spill column n2 times W_N^{-n2 k1}, inverse DFT
    // (unscaled), x[n1] = z(n1 N2 + n2) N.
    __device__ static __forceinline__ void reg_unspill(const KP &k, cf (&x)[N1], int pr, int64_t n2) {
        static_assert(kRegCols, "register columns only");
        const Buf Y(k.Yd + (int64_t)pr * pstride(k), (uint32_t)(pstride(k) * 8));
        const uint32_t RP = (uint32_t)rpitch(k);
        const float invN = k.invN;
#pragma unroll
        for (int k1 = 0; k1 < N1; ++k1) x[k1] = Y.ld2(((uint32_t)k1 * RP + (uint32_t)n2) * 8u, 0u);
#pragma unroll
        for (int k1 = 1; k1 < N1; ++k1) {
            float rev = (float)((uint32_t)n2 * (uint32_t)k1) * invN;
            if (rev >= 0.5f) rev -= 1.0f;
            x[k1] = cmul(x[k1], expi_rev(rev));
        }
        RegDft<N1, true>::run(x);
    }

    // Fold-mode fast passes (host-selected on the mixed-radix split: fold
    // source, chi2(df != 1) draws by the pair sampler, no injected draws, no
    // null in the epilogue).  Every lane owns one column n2 = n20 + lane and
    // keeps it in registers from the draws to the spill: no LDS at all.  The
    // pair sampler keys samples (2m, 2m + 1) -- columns (n2 & ~1, n2 | 1) of
    // one row -- so the lanes of a column pair split the draws by channel
    // (even lane: channel a, odd lane: channel b, both columns) and swap the
    // halves with one DPP move: every draw once, bitwise the values
    // source4 / epilogue4 produce (test_gpu_configs: fold fast == generic).
    __device__ static __forceinline__ void pair_draws(const Rng &g, uint32_t n, uint32_t cme, bool odd, float df,
                                                      float &va, float &vb) {
        float x0, x1;
        chi2_pair(g, n >> 1, cme, df, x0, x1);
        const float send = odd ? x0 : x1;          // even: a(n2 | 1); odd: b(n2 & ~1)
        const float recv = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(send), 0xB1, 0xF, 0xF, false));
        va = odd ? recv : x0;
        vb = odd ? x1 : recv;
    }
    __device__ static void passA_fold(const KP &k) {
        static_assert(kRegCols, "fold fast pass A: register columns");
        const int tid = threadIdx.x;
        int cbx, pr;
        xcd_block(cbx, pr);
        const int ra = 2 * pr - k.poff, rb = ra + 1;
        const bool hasa = ra >= 0, hasb = rb < k.p.nchan;
        const PssPipeline &p = k.p;
        const uint32_t n2 = (uint32_t)(cbx * B + tid), N2 = (uint32_t)k.N2;
        const uint32_t ca = (uint32_t)(p.chan0 + ra), cb = ca + 1u;
        const bool odd = (tid & 1) != 0;
        const Rng g(p.seed, p.call_gen, P_PULSE);
        const int last = p.prof_rows - 1;
        const int pra = (p.prof_rows == 1) ? 0 : min(max((int)ca - p.prof_row0, 0), last);
        const int prb = (p.prof_rows == 1) ? 0 : min(max((int)cb - p.prof_row0, 0), last);
        const float *pfa = p.prof + (int64_t)pra * p.nph, *pfb = p.prof + (int64_t)prb * p.nph;
        const uint32_t nph = (uint32_t)p.nph;
        const float dn = p.draw_norm, df = p.gen_df;
        cf x[N1];
        uint32_t b = n2 % nph;                       // profile bin of sample n1 N2 + n2
        const uint32_t db = N2 % nph;
        // (compile-time row index: a runtime-indexed x[] would live in scratch)
        static_for<0, N1>([&](auto IC) {
            constexpr int n1 = decltype(IC)::value;
            const uint32_t n = (uint32_t)n1 * N2 + n2;
            float va, vb;
            pair_draws(g, n, odd ? cb : ca, odd, df, va, vb);
            x[n1] = make_float2(hasa ? pfa[b] * va * dn : 0.f, hasb ? pfb[b] * vb * dn : 0.f);
            b += db;
            if (b >= nph) b -= nph;
        });
        reg_spill(k, x, pr, n2);
    }
    __device__ static void passC_fold(const KP &k) {
        static_assert(kRegCols, "fold fast pass C: register columns");
        const int tid = threadIdx.x;
        int cbx, pr;
        xcd_block(cbx, pr);
        const int ra = 2 * pr - k.poff, rb = ra + 1;
        const bool hasa = ra >= 0, hasb = rb < k.p.nchan;
        const PssPipeline &p = k.p;
        const uint32_t n2 = (uint32_t)(cbx * B + tid), N2 = (uint32_t)k.N2;
        const uint32_t ca = (uint32_t)(p.chan0 + ra), cb = ca + 1u;
        const bool odd = (tid & 1) != 0;
        const Rng g(p.seed, p.call_noise, P_NOISE);
        const float invN = k.invN, nn = p.noise_norm, df = p.noise_df;
        // The scaled column is staged in LDS, private to the lane (no
        // barrier): the noise loop may call the rare Marsaglia-Tsang retry,
        // and a whole column held in registers across those calls spills
        // (167 VGPRs of scratch at N1 = 30).
        __shared__ cf sg[N1 * B];                       // [n1][lane]
        {
            cf x[N1];
            reg_unspill(k, x, pr, n2);
#pragma unroll
            for (int n1 = 0; n1 < N1; ++n1) sg[n1 * B + tid] = make_float2(x[n1].x * invN, x[n1].y * invN);
        }
        float *oa = p.data + (int64_t)max(ra, 0) * p.ld, *ob = p.data + (int64_t)min(rb, p.nchan - 1) * p.ld;
#pragma unroll 2
        for (int n1 = 0; n1 < N1; ++n1) {
            const uint32_t n = (uint32_t)n1 * N2 + n2;
            float va, vb;
            pair_draws(g, n, odd ? cb : ca, odd, df, va, vb);
            const cf z = sg[n1 * B + tid];
            if (hasa) oa[n] = fmaf(nn, va, z.x);
            if (hasb) ob[n] = fmaf(nn, vb, z.y);
        }
    }

    // inverse column FFTs of one spilled pair block; result left in LDS in
    // natural order (LdsC::at(column, n1)), unscaled.  The load loop is
    // deliberately rolled: with every load of the block in flight at once
    // (64 KB per workgroup) the column passes overflow the XCD's L2 and the
    // half-line reads / 32-B output segments of neighbouring blocks stop
    // merging (PMC: +19% FETCH, +31% WRITE, pass C 17.6 -> 18.5 ms).
    __device__ static __forceinline__ void inv_block(const KP &k, const cf *Yp, int64_t n20, cf *lds, int tid) {
        __shared__ cf tw16[kTw16Size];
        tw16_fill(tw16, tid, T);     // read after the spill loads' barrier
        const int64_t N2 = k.N2;
        const float invN = k.invN;
        const Buf Y(Yp, (uint32_t)(pstride(k) * 8));   // one pair spill, < 2^28 bytes
        const uint32_t RP = (uint32_t)rpitch(k);
        const uint32_t s0 = (uint32_t)n20 * 8u;        // wave-uniform part of the offset
        {
#pragma unroll 1
        for (int it = tid; it < N1 * B / 4; it += T) {
            const int k1 = it / (B / 4);
            const int b4 = (it - k1 * (B / 4)) * 4;
            const uint32_t off = ((uint32_t)k1 * RP + (uint32_t)b4) * 8u;
            const float4 lo = Y.ld4(off, s0), hi = Y.ld4(off + 16u, s0);
            const cf a[4] = {make_float2(lo.x, lo.y), make_float2(lo.z, lo.w),
                             make_float2(hi.x, hi.y), make_float2(hi.z, hi.w)};
            // W^{m}, m = (n20 + b4 + i) k1 < N (exact in 32-bit and float):
            // W^{(n20 + b4) k1} (W^{k1})^i -- two native sincos per 4 points
            const uint32_t m0 = (uint32_t)(n20 + b4) * (uint32_t)k1;
            float r0 = (float)m0 * invN;
            if (r0 >= 0.5f) r0 -= 1.0f;
            float r1 = (float)k1 * invN;
            if (r1 >= 0.5f) r1 -= 1.0f;
            const cf w0 = expi_rev(r0), w1 = expi_rev(r1);
            const cf w2 = cmul(w1, w1);
            const cf tw[4] = {w0, cmul(w0, w1), cmul(w0, w2), cmul(w0, cmul(w2, w1))};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                lds[LdsC::at(b4 + i, k1)] = cmul(a[i], tw[i]);
            }
        }
        }
        __syncthreads();
        cf v[E];
        if constexpr (kWaveCols) {
            const int wv = tid >> 6, lane = tid & 63;
            cf *wl = lds + wv * LdsC::RS;
            FW::template load<RI0>(v, wl, lane);
            stage_sync<true>();
            FW::template run_tw<true, 1, I...>(v, wl, lane, tw16);
            FW::template store<RIL>(v, wl, lane);
        } else {
            FF::template load<RI0>(v, lds, tid);
            __syncthreads();
            FF::template run_tw<true, 1, I...>(v, lds, tid, tw16);
            FF::template store<RIL>(v, lds, tid);
        }
        __syncthreads();
    }

    // C: inverse column FFTs of the data pair, then the epilogues of channels
    // a, b straight from LDS (delayed-null decisions from the mask table).
    __device__ static void passC(const KP &k) {
        __shared__ __align__(128) cf lds[B * LdsC::RS];   // (128-B aligned: the FFT's byte-address exchanges)
        const int tid = threadIdx.x;
        int cbx, pr;
        xcd_block(cbx, pr);
        const int ra = 2 * pr - k.poff, rb = ra + 1;
        const bool hasa = ra >= 0, hasb = rb < k.p.nchan;
        const int64_t n20 = (int64_t)cbx * B;
        const bool mask = k.mtab != 0;
        const float invN = k.invN;
        if constexpr (kRegCols) {
            cf x[N1];
            reg_unspill(k, x, pr, n20 + tid);
#pragma unroll
            for (int n1 = 0; n1 < N1; ++n1) lds[LdsC::at(tid, n1)] = x[n1];
            __syncthreads();
        } else {
            inv_block(k, k.Yd + (int64_t)pr * pstride(k), n20, lds, tid);
        }
#pragma unroll 1
        for (int it = tid; it < N1 * B / 4; it += T) {
            const int n1 = it / (B / 4);
            const int b4 = (it - n1 * (B / 4)) * 4;
            const int64_t n = n1 * k.N2 + n20 + b4;
            float da[4], db[4], ma[4], mb[4];
            const uint32_t ha = (mask && hasa) ? mask_bits4<B, N1>(k, ra, cbx, n1, b4) : 0u;
            const uint32_t hb = (mask && hasb) ? mask_bits4<B, N1>(k, rb, cbx, n1, b4) : 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const cf z = lds[LdsC::at(b4 + i, n1)];
                da[i] = z.x * invN;
                db[i] = z.y * invN;
                ma[i] = ((ha >> i) & 1u) ? 2.0f : 0.0f;
                mb[i] = ((hb >> i) & 1u) ? 2.0f : 0.0f;
            }
            if (hasa) epilogue4(k, ra, n, 4, da, ma, false);
            if (hasb) epilogue4(k, rb, n, 4, db, mb, false);
        }
    }

    // C, fast path with register-resident columns: 16 columns of 1024 or 2048
    // points per 512-thread workgroup (64-B output segments per channel row;
    // tools/seg_bw.hip: 64-B write segments run at 5.2 TB/s against 3.1 for
    // 32 B).  Each wave keeps its two columns in registers between three LDS
    // phases --
    // (1) the spill rows in two halves of N1/2 (128-B row segments, twiddled
    // as in inv_block) staged in LDS and picked up into the FFT input mapping,
    // (2) the two wave-local inverse FFTs one after the other through the
    // wave's own LDS row, (3) each channel's scaled outputs staged as
    // [n1][17] floats and stored as whole 64-B row segments with the noise --
    // so the LDS buffer is half a block, one FFT row per wave or one
    // channel's outputs, whichever is largest, not the whole block.
    //   * 2048-point columns (2^24 with a delayed null): the whole block
    //     would be 256 KB and cannot sit in LDS at all; 139 392 B here, 128
    //     VGPRs of columns per lane (k_pairC_fast32 at 2 waves per SIMD), one
    //     workgroup per CU.
    //   * 1024-point columns (2^22, 2^23, C5's 1024 x 16384): passC_fast's
    //     139 392-B block leaves one 1024-thread workgroup per CU, every barrier
    //     putting all 16 waves of the CU in the same phase; 69 760 B + tw16 =
    //     71 936 B here and 64 VGPRs of columns (4 waves per SIMD, the
    //     128-VGPR cap: 94 used, no scratch), so two workgroups share a CU and
    //     one loads or stores while the other transforms.
    // Bitwise the values of passC_fast (same twiddles, FFT and epilogue).
    //
    // NULLC (1024-point columns with the mask table; plan token C:null): the
    // samples the table nulls for EVERY f are nulled here, in the staging,
    // instead of being stored and then rewritten by the fix-up.  Each thread
    // takes the 16-bit window of the table's always bits (mt_bits[].x, no
    // root records, no f-dependent branch) of its two rows' 16-sample
    // segments, for both channels, at the start of the kernel; next to a
    // channel's staging writes every non-zero nibble appends one 16-bit
    // entry {n1:10, c4/4:2, nibble:4} to an LDS list (a ballot prefix and one
    // LDS atomic per wave; the list holds the whole block, 4096 entries, so
    // it cannot overflow).  After the staging barrier the list is
    // walked densely -- the replacement draws cost what the nulled fraction
    // costs, not one divergent branch per wave -- and overwrites the staged
    // value with vr * sc; the store loop then adds the noise it draws anyway:
    // fmaf(nn, vn, vr * sc), the fix-up's expression and bits.  Every sample
    // is still stored, as whole 64-B segments.  The f-dependent positions
    // (~1 %) are left to k_null_fix_list<true>.  80 136 B of LDS: two
    // workgroups still share a CU.
    template <bool NULLC = false>
    __device__ static void passC_fast32(const KP &k) {
        static_assert((N1 == 1024 || N1 == 2048) && (T == 1024 || T == 512) && B % (T / 64) == 0 &&
                      kWaveCols == false, "register-resident wide pass C: 2^m columns of 1024 / 2048");
        constexpr int NW = T / 64, CPW = B / NW;        // waves, columns per wave
        constexpr int E1 = N1 / 64;                     // values per lane of one column
        constexpr int H = N1 / 2;                       // rows per load half
        constexpr int RSH = H + H / 16 + 1;             // padded pitch of a half column (odd)
        constexpr int OSP = B + 1;                      // staging pitch (floats)
        using LW = Lds<N1, -1>;                         // FFT rows: padded, as passC_fast's
        using FWC = Fft<N1, 1, 64, true, -1>;
        constexpr int RI0 = FWC::template first<I...>();
        constexpr int LRI = N1 / RI0;                   // input mapping: v[ib RI0 + q] = lane + 64 ib + LRI q
        constexpr int B1 = B * RSH * 8, B2 = NW * LW::RS * 8, B3 = N1 * OSP * 4;
        constexpr int BUF = (B1 > B2 ? B1 : B2) > B3 ? (B1 > B2 ? B1 : B2) : B3;
        __shared__ __align__(16) char smem[BUF];
        __shared__ cf tw16[kTw16Size];
        static_assert(!NULLC || (N1 == 1024 && T == 512 && B == 16), "NULLC: two rows per thread, 16-bit entries");
        // (NULLC only; unused and not allocated otherwise) the nulled items of
        // the channel being staged, and their count per channel
        __shared__ uint16_t nlist[NULLC ? N1 * B / 4 : 1];
        __shared__ uint32_t ncount[2];
        const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
        tw16_fill(tw16, tid, T);
        if constexpr (NULLC) {
            if (tid < 2) ncount[tid] = 0u;              // (phase 1's barriers come before its first use)
        }
        int cbx, pr;
        xcd_block(cbx, pr);
        const int ra = 2 * pr - k.poff, rb = ra + 1;
        const bool hasa = ra >= 0, hasb = rb < k.p.nchan;
        const int64_t N2 = k.N2;
        const PssPipeline &p = k.p;
        const float invN = k.invN, nn = p.noise_norm;
        const int64_t n20 = (int64_t)cbx * B;
        const Buf Y(k.Yd + (int64_t)pr * pstride(k), (uint32_t)(pstride(k) * 8));
        const uint32_t RP = (uint32_t)rpitch(k);
        cf *hb = reinterpret_cast<cf *>(smem);
        cf v[CPW][E1];
        // NULLC: the always bits of rows tid, tid + T of both channels --
        // table positions p0 .. p0 + 15, p0 = (n1 N2 + n20 - is) mod N, in
        // two table words (the second wraps with the table).  Loaded here,
        // ahead of the spill rows, and packed into one register per channel
        // after phase 1: loaded where phase 3 uses them, the ramp word and
        // then the table words were two exposed latencies per channel.
        uint32_t mlo[2][N1 / T] = {}, mhi[2][N1 / T] = {}, msh[2][N1 / T] = {}, nwin[2] = {0u, 0u};
        if constexpr (NULLC) {
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                if (ch ? hasb : hasa) {                 // (uniform; the edge pairs' missing channel has no ramp word)
                    uint32_t is;
                    float tf;
                    mask_split((uint64_t)p.mask_ramp[ch ? rb : ra], k.log2n, is, tf);
                    const uint32_t nm = (uint32_t)k.N - 1u, wm = nm >> 5;
                    const uint32_t *ax = reinterpret_cast<const uint32_t *>(k.mt_bits);   // .x of word w: ax[2 w]
#pragma unroll
                    for (int j = 0; j < N1 / T; ++j) {
                        const uint32_t p0 = ((uint32_t)(tid + j * T) * (uint32_t)N2 + (uint32_t)n20 - is) & nm;
                        const uint32_t w = p0 >> 5;
                        PSS_DASSERT(w <= wm);
                        mlo[ch][j] = ax[2u * w];
                        mhi[ch][j] = ax[2u * ((w + 1u) & wm)];
                        msh[ch][j] = p0 & 31u;
                    }
                }
            }
        }
        // The 1024-point form runs at the 128-VGPR cap (two workgroups per
        // CU) with 64 VGPRs of columns: each phase takes its thread indices
        // through opaque(), so that address arithmetic of a later phase (or of
        // the second column's FFT, identical to the first's) is recomputed
        // where it is used instead of being held in registers -- spilled --
        // across the FFTs (as PairRowsSeq).
        auto fresh = [](int x) __attribute__((always_inline)) { return N1 == 1024 ? opaque(x) : x; };
        // (1) spill rows, two halves
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (h) __syncthreads();                     // the first half has been picked up
#pragma unroll 1
            for (int it = tid; it < H * B / 4; it += T) {
                const int k1l = it / (B / 4), b4 = (it - k1l * (B / 4)) * 4;
                const int k1 = h * H + k1l;
                const uint32_t off = ((uint32_t)k1 * RP + (uint32_t)b4) * 8u, so = (uint32_t)n20 * 8u;
                const float4 lo = Y.ld4(off, so), hi = Y.ld4(off + 16u, so);
                const cf a[4] = {make_float2(lo.x, lo.y), make_float2(lo.z, lo.w),
                                 make_float2(hi.x, hi.y), make_float2(hi.z, hi.w)};
                // the twiddles of inv_block, bit for bit
                const uint32_t m0 = (uint32_t)(n20 + b4) * (uint32_t)k1;
                float r0 = (float)m0 * invN;
                if (r0 >= 0.5f) r0 -= 1.0f;
                float r1 = (float)k1 * invN;
                if (r1 >= 0.5f) r1 -= 1.0f;
                const cf w0 = expi_rev(r0), w1 = expi_rev(r1);
                const cf w2 = cmul(w1, w1);
                const cf tw[4] = {w0, cmul(w0, w1), cmul(w0, w2), cmul(w0, cmul(w2, w1))};
#pragma unroll
                for (int i = 0; i < 4; ++i) hb[(b4 + i) * RSH + k1l + (k1l >> 4)] = cmul(a[i], tw[i]);
            }
            __syncthreads();
            // the FFT input mapping: register i = ib RI0 + q holds position
            // lane + 64 ib + LRI q (the half it lies in is compile-time)
#pragma unroll
            for (int i = 0; i < E1; ++i) {
                const int pc = 64 * (i / RI0) + LRI * (i % RI0);      // position minus lane
                if (pc / H != h) continue;
                const int pl = lane + pc - h * H;
#pragma unroll
                for (int c = 0; c < CPW; ++c) v[c][i] = hb[(wv + NW * c) * RSH + pl + (pl >> 4)];
            }
        }
        __syncthreads();
        if constexpr (NULLC) {
#pragma unroll
            for (int ch = 0; ch < 2; ++ch)
#pragma unroll
                for (int j = 0; j < N1 / T; ++j)
                    nwin[ch] |= ((uint32_t)(((((uint64_t)mhi[ch][j]) << 32) | mlo[ch][j]) >> msh[ch][j]) & 0xffffu)
                                << (16 * j);
        }
        // (2) the inverse column FFTs through the wave's own LDS row
        {
            cf *wl = reinterpret_cast<cf *>(smem) + wv * LW::RS;
#pragma unroll
            for (int c = 0; c < CPW; ++c) {
                if (c) stage_sync<true>();
                FWC::template run_tw<true, 1, I...>(v[c], wl, fresh(lane), tw16);
            }
        }
        // (3) per channel: stage the scaled outputs, store rows with the noise
        constexpr int RIL = FWC::template last_of<I...>();
        float *stg = reinterpret_cast<float *>(smem);
        const uint32_t ca = (uint32_t)(p.chan0 + ra), cb = ca + 1u;
        const Rng gn(p.seed, p.call_noise, P_NOISE);
        const uint32_t rbytes = (uint32_t)(k.N * 4);
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            __syncthreads();                            // FFT rows / previous channel's staging free
            const int sl = fresh(lane);
#pragma unroll
            for (int i = 0; i < E1; ++i) {
                int bb, pos;
                FWC::template where<RIL>(i, sl, bb, pos);
#pragma unroll
                for (int c = 0; c < CPW; ++c) stg[pos * OSP + wv + NW * c] = (ch ? v[c][i].y : v[c][i].x) * invN;
            }
            if constexpr (NULLC) {
                if (ch ? hasb : hasa) {
                    // entries of this thread (at most 2 x 4), compacted over the
                    // wave: the exclusive prefix of the counts from four ballots
                    uint32_t win[N1 / T], cnt = 0;
#pragma unroll
                    for (int j = 0; j < N1 / T; ++j) {
                        win[j] = (nwin[ch] >> (16 * j)) & 0xffffu;
#pragma unroll
                        for (int g = 0; g < 4; ++g) cnt += ((win[j] >> (4 * g)) & 15u) ? 1u : 0u;
                    }
                    const uint64_t below = (1ull << lane) - 1ull;
                    uint32_t e = 0, total = 0;
#pragma unroll
                    for (int bit = 0; bit < 4; ++bit) {
                        const uint64_t bal = __ballot((cnt >> bit) & 1u);
                        e += (uint32_t)__popcll(bal & below) << bit;
                        total += (uint32_t)__popcll(bal) << bit;
                    }
                    uint32_t b0 = 0;
                    if (lane == 0 && total) b0 = atomicAdd(&ncount[ch], total);
                    e += (uint32_t)__shfl((int)b0, 0);
                    const uint32_t r0 = (uint32_t)fresh(tid);
#pragma unroll
                    for (int j = 0; j < N1 / T; ++j) {
#pragma unroll
                        for (int g = 0; g < 4; ++g) {
                            const uint32_t h = (win[j] >> (4 * g)) & 15u;
                            if (h) {
                                PSS_DASSERT(e < (uint32_t)(N1 * B / 4));
                                nlist[e++] = (uint16_t)(((r0 + (uint32_t)(j * T)) << 6) | ((uint32_t)g << 4) | h);
                            }
                        }
                    }
                }
            }
            __syncthreads();
            const bool has = ch ? hasb : hasa;
            if (!has) continue;                         // (uniform)
            const uint32_t c = ch ? cb : ca;
            if constexpr (NULLC) {
                // the listed items, densely: replacement draws of the set bits
                // over the staged values (disjoint items: any order)
                const uint32_t ne = ncount[ch];
                const Rng gr(p.seed, p.call_null, P_REP);
                const float sc = p.null_rep_scale;
                for (uint32_t e = (uint32_t)fresh(tid); e < ne; e += (uint32_t)T) {
                    const uint32_t d = nlist[e], n1 = d >> 6, c4 = ((d >> 4) & 3u) * 4u;
                    const uint32_t nb = n1 * (uint32_t)N2 + (uint32_t)n20 + c4;
                    PSS_DASSERT(n1 < (uint32_t)N1 && (int64_t)nb + 4 <= k.N);
                    const float4 xr = chi2_1x4(gr.bits(nb >> 2, c, 0u));
                    float *sr = stg + n1 * OSP + c4;
                    if (d & 1u) sr[0] = xr.x * sc;
                    if (d & 2u) sr[1] = xr.y * sc;
                    if (d & 4u) sr[2] = xr.z * sc;
                    if (d & 8u) sr[3] = xr.w * sc;
                }
                __syncthreads();
            }
            const Buf o(p.data + (int64_t)(ch ? rb : ra) * p.ld, rbytes);
            const int t0 = fresh(tid);
#pragma unroll
            for (int t = 0; t < N1 * B / 4 / T; ++t) {
                const int it = t0 + t * T;
                const int n1 = it / (B / 4), c4 = (it - n1 * (B / 4)) * 4;
                const uint32_t n = (uint32_t)(n1 * (int)N2) + (uint32_t)n20 + (uint32_t)c4;
                const float4 x = chi2_1x4(gn.bits(n >> 2, c, 0u));
                const float *sr = stg + n1 * OSP + c4;
                o.st4(fmaf(nn, x.x, sr[0]), fmaf(nn, x.y, sr[1]), fmaf(nn, x.z, sr[2]), fmaf(nn, x.w, sr[3]),
                      n * 4u, 0);
            }
        }
    }

    // C, fast path (host-selected: Philox draws with df = 1 for the noise, no
    // injected draws, no observe() copy), the whole column block in LDS.
    // Bitwise equal to passC: every sample is stored as signal + noise; a
    // delayed null's samples are rewritten afterwards by k_null_fix_list
    // (fusing the table lookups here measured 27.0 ms against 16.6 + 2.5 for
    // pass C + fix-up, round 2).
    __device__ static void passC_fast(const KP &k) {
        static_assert(kItemsExact, "fast pass C: whole items per thread");
        __shared__ __align__(128) cf lds[B * LdsC::RS];
        const int tid = threadIdx.x;
        int cbx, pr;
        xcd_block(cbx, pr);
        const int ra = 2 * pr - k.poff, rb = ra + 1;
        const bool hasa = ra >= 0, hasb = rb < k.p.nchan;
        const int64_t N2 = k.N2;
        const PssPipeline &p = k.p;
        const float invN = k.invN, nn = p.noise_norm;
        const uint32_t ca = (uint32_t)(p.chan0 + ra), cb = ca + 1u;
        const Rng gn(p.seed, p.call_noise, P_NOISE);
        const uint32_t rbytes = (uint32_t)(k.N * 4);
        const Buf oa(p.data + (int64_t)max(ra, 0) * p.ld, rbytes), ob(p.data + (int64_t)min(rb, p.nchan - 1) * p.ld, rbytes);
        const int64_t n20 = (int64_t)cbx * B;
        if constexpr (kRegCols) {
            // register columns (mixed radix, N1 = 12 .. 60): the inverse of
            // passC -- reg_unspill's per-element twiddles and RegDft, not
            // inv_block's LDS transform with composed twiddles, whose
            // roundings differ in the last bit
            cf x[N1];
            reg_unspill(k, x, pr, n20 + tid);
#pragma unroll
            for (int n1 = 0; n1 < N1; ++n1) lds[LdsC::at(tid, n1)] = x[n1];
            __syncthreads();
        } else {
            inv_block(k, k.Yd + (int64_t)pr * pstride(k), n20, lds, tid);
        }
        float acc[ITEMS][2][4];
#pragma unroll
        for (int t = 0; t < ITEMS; ++t) {
            const int it = tid + t * T;
            const int n1 = it / (B / 4);
            const int b4 = (it - n1 * (B / 4)) * 4;
            const uint32_t n = (uint32_t)(n1 * (int)N2) + (uint32_t)n20 + (uint32_t)b4;   // N <= 2^24
            const float4 xa = chi2_1x4(gn.bits(n >> 2, ca, 0u));
            const float4 xb = chi2_1x4(gn.bits(n >> 2, cb, 0u));
            const float na[4] = {xa.x, xa.y, xa.z, xa.w}, nb[4] = {xb.x, xb.y, xb.z, xb.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const cf z = lds[LdsC::at(b4 + i, n1)];
                acc[t][0][i] = fmaf(nn, na[i], z.x * invN);
                acc[t][1][i] = fmaf(nn, nb[i], z.y * invN);
            }
        }
        // (a delayed null's samples are rewritten afterwards: k_null_fix_list)
#pragma unroll
        for (int t = 0; t < ITEMS; ++t) {
            const int it = tid + t * T;
            const int n1 = it / (B / 4);
            const int b4 = (it - n1 * (B / 4)) * 4;
            const uint32_t off = ((uint32_t)(n1 * (int)N2) + (uint32_t)n20 + (uint32_t)b4) * 4u;
            if (hasa) oa.st4(acc[t][0][0], acc[t][0][1], acc[t][0][2], acc[t][0][3], off, 0);
            if (hasb) ob.st4(acc[t][1][0], acc[t][1][1], acc[t][1][2], acc[t][1][3], off, 0);
        }
    }

    // Mask table build: inverse column FFTs of node pair `blockIdx.y`, stored
    // (scaled) as node rows nodes[2 pr], nodes[2 pr + 1].
    __device__ static void node_col(const KP &k, float *nodes) {
        __shared__ __align__(128) cf lds[B * LdsC::RS];   // (128-B aligned: the FFT's byte-address exchanges)
        const int tid = threadIdx.x;
        int cbx, pr;
        xcd_block(cbx, pr);
        const int64_t n20 = (int64_t)cbx * B;
        const float invN = k.invN;
        inv_block(k, k.Ym + (int64_t)pr * pstride(k), n20, lds, tid);
        float *ra = nodes + (int64_t)(2 * pr) * k.N, *rb = ra + k.N;
        for (int it = tid; it < N1 * B / 4; it += T) {
            const int n1 = it / (B / 4);
            const int b4 = (it - n1 * (B / 4)) * 4;
            const int64_t n = n1 * k.N2 + n20 + b4;
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const cf z = lds[LdsC::at(b4 + i, n1)];
                a[i] = z.x * invN;
                b[i] = z.y * invN;
            }
            *reinterpret_cast<float4 *>(ra + n) = make_float4(a[0], a[1], a[2], a[3]);
            *reinterpret_cast<float4 *>(rb + n) = make_float4(b[0], b[1], b[2], b[3]);
        }
    }
};

template <typename C, int T>
__global__ __launch_bounds__(T) void k_pairA(KP k) { C::template passA<false>(k); }
template <typename C, int T, bool SHARED>
__global__ __launch_bounds__(T) void k_pairA_fast(KP k) { C::template passA<true, SHARED>(k); }
template <typename C>
__global__ __launch_bounds__(256) void k_prof_cols(KP k, float4 *out) { C::prof_cols(k, out); }
template <typename C, int T>
__global__ __launch_bounds__(T) void k_pairC(KP k) { C::passC(k); }
template <typename C, int T>
__global__ __launch_bounds__(T) void k_pairC_fast(KP k) { C::passC_fast(k); }
// W: min waves per SIMD.  512 threads at 2 (256 VGPRs) for the 2048-point
// columns (64 complex values per lane); at 4 (128 VGPRs) for the 1024-point
// columns, whose 72 KB of LDS then lets two workgroups share a CU.
template <typename C, int T, int W = (T == 512 ? 2 : 4)>
__global__ __launch_bounds__(T, W) void k_pairC_fast32(KP k) { C::passC_fast32(k); }
// the 1024-point form that also nulls the always-nulled samples (NULLC)
template <typename C>
__global__ __launch_bounds__(512, 4) void k_pairC_null(KP k) { C::template passC_fast32<true>(k); }
template <typename C, int T>
__global__ __launch_bounds__(T) void k_node_col(KP k, float *nodes) { C::node_col(k, nodes); }
// (4 waves per SIMD for columns up to 30: the compiler would otherwise keep
// every row's draws in flight at once, 210 VGPRs for N1 = 30)
template <typename C, int T>
__global__ __launch_bounds__(T, C::kFoldWaves) void k_pairA_fold(KP k) { C::passA_fold(k); }
template <typename C, int T>
__global__ __launch_bounds__(T, C::kFoldWavesC) void k_pairC_fold(KP k) { C::passC_fold(k); }

// Extra LDS row pitch of the column kernels (tools/lds_banks.py): pass A's
// spill-store loop reads 4 columns x 16 rows per 32-lane group (a 32/B pitch
// offset spreads the columns over the 64 read banks); pass C's load loop
// writes 4 columns x 4 rows per 16-lane group (16/B over the 32 write banks).
// B < 32: a pitch that is a multiple of 16 complex, so the wave-local column
// FFTs get the byte-address exchanges (Fft::XB: round 2's 4-complex pad cost
// ~100 address VALU per lane in pass A); the spill-store loop then reads 32
// consecutive rows of one 4-column group per 32-lane group (conflict-free at
// any pitch, passA).
constexpr int xrs_read(int B) { return B >= 32 ? 1 : 16; }

// ---------------------------------------------------------------------------
// The splits.  A split N1 x N2 is one type, Split<column engine, row engine>;
// the launchers below take nothing else.
// ---------------------------------------------------------------------------
// Column engine: N1-point columns in blocks of B on T threads, radix lists CF
// (forward) and CI (inverse).
template <int N1_, int B_, int T_, typename CF, typename CI>
struct ColEngine {
    static constexpr int N1 = N1_, B = B_, T = T_;
    using PC = PairCols<N1, B, T, CF, CI, xrs_read(B)>;   // pass A, generic pass C
    // the LDS-resident fast pass C (passC_fast) and the 16-column register-
    // resident one of the 1024- and 2048-point columns (passC_fast32): the
    // padded layout (pass C measured 0.5 ms faster on it at C3: its transposes
    // gain nothing from the swizzle and the XOR addressing costs VALU)
    using PCFast = PairCols<N1, B, T, CF, CI, -1>;
    using PCFast32 = PairCols<N1, 16, 512, CF, CI, -1>;
    // 128 columns per workgroup: the lane-private LDS staging of the column
    // (N1 x 8 B per lane) then allows ~5 workgroups per CU
    static constexpr int FB = B > 128 ? 128 : B;
    using PCFold = PairCols<N1, FB, FB, CF, CI>;
    using PCNode = PairCols<N1, B, T, CF, CI>;            // the mask table's node shifts
    using MaskCols = Cols<N1, B, T, CF>;                  // the mask spectrum's forward half
};
// Power-of-two columns: B * N1 = 8192 complex per workgroup up to 512 points,
// 8-column blocks above; column inverses reuse the forward list.
template <int N1>
struct Pow2Cols;
template <> struct Pow2Cols<16> : ColEngine<16, 512, 512, C16, C16> {};
template <> struct Pow2Cols<32> : ColEngine<32, 256, 512, C32F, C32F> {};
template <> struct Pow2Cols<64> : ColEngine<64, 128, 512, C64F, C64F> {};
template <> struct Pow2Cols<128> : ColEngine<128, 64, 512, C128F, C128F> {};
template <> struct Pow2Cols<256> : ColEngine<256, 32, 512, C256, C256> {};
template <> struct Pow2Cols<512> : ColEngine<512, 16, 512, C512F, C512F> {};
template <> struct Pow2Cols<1024> : ColEngine<1024, 8, 512, C1kF, C1kF> {};
template <> struct Pow2Cols<2048> : ColEngine<2048, 8, 512, C2kF, C2kF> {};
// Register columns of the mixed-radix splits: one column per thread, B = T.
template <int N1, typename CF, typename CI, int T>
using RegCols = ColEngine<N1, T, T, CF, CI>;

// Row engine: the two N2-point rows of a pair on TR threads (PairRows), one
// row at a time on TS (PairRowsSeq), the mask spectrum's single rows on TRF.
template <int N2_, int TR_, typename RF, typename RI, int TRF_>
struct RowEngine {
    static constexpr int N2 = N2_, TR = TR_, TRF = TRF_;
    using PR = PairRows<N2, TR, RF, RI>;
    // 16 values of each row per thread (16384-point rows: 512 threads with
    // 32 measured 47.8 against 43.9 ms at C5, profiles/r05/r16/)
    static constexpr int TS = N2 / 16;
    using PRS = PairRowsSeq<N2, TS, RF, RI>;
    using MaskRows = Rows<N2, 1, TRF, RF>;
};
template <int N2>
struct RowsOf;
template <> struct RowsOf<1024> : RowEngine<1024, 128, C1kF, C1kI, 64> {};
template <> struct RowsOf<2048> : RowEngine<2048, 256, C2kF, C2kI, 128> {};
template <> struct RowsOf<4096> : RowEngine<4096, 512, C4k, C4k, 256> {};
template <> struct RowsOf<8192> : RowEngine<8192, 1024, C8kF, C8kI, 512> {};
template <> struct RowsOf<16384> : RowEngine<16384, 1024, C16kF, C16kI, 1024> {};
template <> struct RowsOf<2500> : RowEngine<2500, 250, RList<5, 5, 5, 5, 4>, RList<4, 5, 5, 5, 5>, 250> {};

template <typename C, typename R>
struct Split : C, R {
    // the mask table's position arithmetic is for N = 2^m (validate() sends
    // delayed nulls of other lengths to the direct path)
    static constexpr bool kMaskTable = (C::N1 & (C::N1 - 1)) == 0 && R::N2 <= 8192;
};
template <int N1, int N2>
using Pow2Split = Split<Pow2Cols<N1>, RowsOf<N2>>;

// Mask table of a delayed null (see the comment above KCH): mask spectrum,
// KCH node shifts (KCH/2 pair rows through the row and column engines),
// Chebyshev coefficients + classification.  Once per run, channel independent.
template <typename S>
static inline int build_mask_table(KP &k, hipStream_t st, const float *mask_row, char *w, const WsLayout &L) {
    constexpr int N1 = S::N1, N2 = S::N2, B = S::B, T = S::T, TR = S::TR, TRF = S::TRF;
    using PC = typename S::PCNode;
    using PR = typename S::PR;
    cf *mspec = reinterpret_cast<cf *>(w + L.mspec);
    uint32_t *counter = reinterpret_cast<uint32_t *>(w + L.misc);
    uint64_t *nramp = reinterpret_cast<uint64_t *>(w + L.misc + 64);
    float *nnyq = reinterpret_cast<float *>(w + L.misc + 192);
    float *nodes = reinterpret_cast<float *>(w + L.nodes);
    int log2n = 0;
    while ((1ll << log2n) < k.N) ++log2n;
    // spectrum of the (channel independent) mask row
    KP km = k;
    km.p.nchan = 1;
    km.p.chan0 = 0;
    km.p.data = const_cast<float *>(mask_row);
    km.p.ld = k.N;
    km.p.src = PSS_SRC_LOAD;
    km.p.null_mode = PSS_NULL_NONE;
    km.p.data_in_fft = 1;
    km.p.work = mspec;
    using C1 = typename S::MaskCols;
    using R1 = typename S::MaskRows;
    k_colA<C1, T><<<dim3((unsigned)(N2 / B), 1), dim3(T), 0, st>>>(km);
    LAUNCHCHK();
    k_row<R1, TRF><<<dim3((unsigned)N1, 1), dim3(TRF), 0, st>>>(km);
    LAUNCHCHK();
    // node shifts
    if (const int rc = launch_node_params(nramp, nnyq, log2n, st)) return rc;
    KP kn = k;
    kn.p.nchan = KCH;
    kn.p.chan0 = 0;
    kn.p.ramp = nramp;
    kn.p.nyq_re = nnyq;
    kn.p.nyq_im = nnyq;
    kn.poff = 0;
    kn.npairs = KCH / 2;
    kn.Ym = reinterpret_cast<cf *>(w + L.ynode);
    kn.Mspec = mspec;
    k_node_row<PR, TR><<<dim3((unsigned)(KCH / 2), (unsigned)(N1 / 2)), dim3(TR), 0, st>>>(kn);
    LAUNCHCHK();
    k_node_col<PC, T><<<dim3((unsigned)(N2 / B), (unsigned)(KCH / 2)), dim3(T), 0, st>>>(kn, nodes);
    LAUNCHCHK();
    // table
    HIPCHK(hipMemsetAsync(counter, 0, 4, st));
    k.mt_bits = reinterpret_cast<const uint2 *>(w + L.bits);
    k.mt_base = reinterpret_cast<const uint32_t *>(w + L.base);
    k.mt_coef = reinterpret_cast<const float *>(w + L.coef);
    if (const int rc = launch_mask_table(nodes, k.N, reinterpret_cast<uint2 *>(w + L.bits),
                                         reinterpret_cast<uint32_t *>(w + L.base), reinterpret_cast<float *>(w + L.coef),
                                         counter, st))
        return rc;
    {
        uint32_t *wl = reinterpret_cast<uint32_t *>(w + L.wlist);
        uint32_t *wcount = reinterpret_cast<uint32_t *>(w + L.misc + 8);
        const uint32_t nwords = (uint32_t)(k.N / 32);
        // (the f-dependent words' list and count: WsLayout::wlist_f)
        uint32_t *wlf = reinterpret_cast<uint32_t *>(w + L.wlist_f);
        uint32_t *wcount_f = reinterpret_cast<uint32_t *>(w + L.wcount_f);
        HIPCHK(hipMemsetAsync(wcount, 0, 8, st));           // both counts (misc + 8, misc + 12)
        if (const int rc = launch_mask_words(k.mt_bits, nwords, wl, wcount, wlf, wcount_f, st)) return rc;
        k.wlist = wl;
        k.nwlist = wcount;
    }
    k.mtab = 1;
    plan_note(" N:table");
    k.log2n = log2n;
    if (k.p.data_in_fft && !fast_epilogue(k)) {   // generic pass C reads the decisions as bits
        k.mbB = B;
        uint32_t *bm = reinterpret_cast<uint32_t *>(w + L.mbits);
        if (const int rc = launch_mask_bits(k, bm, st)) return rc;
        k.mbits = bm;
    }
    return PSS_OK;
}

// The device's side streams.  Only s[0] (the mask table's) and the events 30
// (fork from the main stream) and 31 (table ready) are in use; allocating
// just those measured inside the C3 step's run-to-run spread in two jobs of
// three and 0.1-0.2 ms above it in one (profiles/fourstep_launcher/), so the
// allocation stays as it was.
struct SideStreams {
    hipStream_t s[2];
    hipEvent_t ev[40];
    bool ok;
};
SideStreams *side_streams();

// The mask table on the side stream, forked from st here (ss), or in line on
// st (no ss); k.mask_ready is what its first reader on st has to wait for.
template <typename S>
static int fork_mask_table(KP &k, hipStream_t st, SideStreams *ss, const float *mask_row, char *w, const WsLayout &L) {
    if (ss) {
        HIPCHK(hipEventRecord(ss->ev[30], st));
        HIPCHK(hipStreamWaitEvent(ss->s[0], ss->ev[30], 0));
    }
    if (const int rc = build_mask_table<S>(k, ss ? ss->s[0] : st, mask_row, w, L)) return rc;
    if (ss) {
        HIPCHK(hipEventRecord(ss->ev[31], ss->s[0]));
        k.mask_ready = ss->ev[31];
    }
    return PSS_OK;
}

// Channel count up to which the side-stream mask table forks after pass A
// (beside the row pass) instead of before it (beside pass A): it costs the
// pass it runs beside ~0.4 ms either way, which at 2048 channels is even
// (46.84-46.89 vs 46.86-47.06 ms per C3 step), at 1024 channels slightly
// better after pass A (kernels 23.05-23.12 vs 23.17-23.20 ms) and at 256
// channels -- a short pass A it slowed by a quarter -- 0.12 ms per step less
// after pass A (6.52-6.56 vs 6.64-6.68 ms, profiles/r06/ab_mask/)
static constexpr int kMaskAfterANchan = 1024;

// One pair range through a split, top to bottom: [mask table], ramp table,
// pass A, [mask table], row pass, pass C, [null fix-up].
template <typename S>
static int launch_pair(KP &k, hipStream_t st, const float *mask_row) {
    constexpr int N1 = S::N1, N2 = S::N2, B = S::B, T = S::T, TR = S::TR;
    using PC = typename S::PC;
    using PR = typename S::PR;
    plan_note(" %dx%d", N1, N2);
    k.poff = k.p.chan0 & 1;
    k.npairs = (k.p.nchan + k.poff + 1) / 2;
    char *w = reinterpret_cast<char *>(k.p.work);
    const WsLayout L = ws_layout(k.p.nchan, k.N);
    k.Yd = reinterpret_cast<cf *>(w + L.yd);
    const bool table = k.p.null_mode == PSS_NULL_DELAYED;
    if (table && !S::kMaskTable)
        return fail(PSS_EUNSUPPORTED, "delayed null on the mixed-radix or 16384-row four-step (N=%lld)",
                    (long long)k.N);
    // With the data in the FFT and the fast passes, nothing reads the table
    // before the null fix-up: build it on a side stream next to pass A or the
    // row pass (its dozen small launches then cost no time on the main
    // stream); the fix-up waits for it.
    SideStreams *ss = table && k.p.data_in_fft ? side_streams() : nullptr;
    const bool table_after_a = ss && k.p.nchan <= kMaskAfterANchan;
    if constexpr (S::kMaskTable) {
        if (table && !table_after_a)
            if (const int rc = fork_mask_table<S>(k, st, ss, mask_row, w, L)) return rc;
    }
    if (!k.p.data_in_fft) {
        // only the null mask was delayed: one elementwise pass with table lookups
        return launch_elementwise(k, st);
    }
    if (!k.p.htab) {   // (a transfer-function run has no ramps)
        cf *rt = reinterpret_cast<cf *>(w + L.rtab);
        k_pair_tab<PR::RFL><<<dim3((unsigned)k.npairs), dim3(64), 0, st>>>(k.p.ramp, k.N, k.p.nchan, k.poff,
                                                                          k.npairs, rt);
        LAUNCHCHK();
        k.rtab = rt;
    }

    const dim3 gc((unsigned)(N2 / B), (unsigned)k.npairs);
    tk_begin(TK_COLA, st);
    // (each `if constexpr` keeps a kernel the column engine does not have
    // from being instantiated; its branch is not reached then)
    const bool fold_a = PC::kRegCols && fold_source(k.p);
    const bool fast_a = !fold_a && PC::kItemsExact && fast_source(k.p);
    if (fold_a) {
        if constexpr (PC::kRegCols) k_pairA_fold<PC, T><<<gc, dim3(T), 0, st>>>(k);
        plan_note(" A:fold");
    } else if (fast_a && k.p.prof_rows == 1) {
        // the shared profile at every sample, once per run (PairCols::prof_cols)
        if constexpr (PC::kItemsExact) {
            float4 *pcol = reinterpret_cast<float4 *>(w + L.pcol);
            const int64_t ne = k.N / 4;
            k_prof_cols<PC><<<dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st>>>(k, pcol);
            LAUNCHCHK();
            k.pcol = pcol;
            k_pairA_fast<PC, T, true><<<gc, dim3(T), 0, st>>>(k);
        }
        plan_note(" A:fast_shared");
    } else if (fast_a) {
        if constexpr (PC::kItemsExact) k_pairA_fast<PC, T, false><<<gc, dim3(T), 0, st>>>(k);
        plan_note(" A:fast");
    } else {
        k_pairA<PC, T><<<gc, dim3(T), 0, st>>>(k);
        plan_note(" A:generic");
    }
    tk_end(st);
    LAUNCHCHK();
    if constexpr (S::kMaskTable) {
        if (table_after_a)
            if (const int rc = fork_mask_table<S>(k, st, ss, mask_row, w, L)) return rc;
    }

    tk_begin(TK_ROW, st);
    const dim3 gr((unsigned)k.npairs, (unsigned)(N1 / 2));
    const bool plain = !k.p.htab && !k.p.tail_a;
    if (N2 > 8192 || (N2 == 8192 && plain)) {
        // one row at a time (PairRowsSeq): the plain runs on 8192-point rows,
        // and the 16384-point rows (C5's 1024 x 16384 split), which have no
        // transfer function / tail variant (run_fourstep keeps those runs on
        // the 2048 x 8192 split)
        if (!plain) return fail(PSS_EUNSUPPORTED, "%d-point rows: no transfer function", N2);
        if constexpr (N2 >= 8192) {
            using PRS = typename S::PRS;
            constexpr int TS = S::TS;
            k_pair_row_seq<PRS, TS, false><<<dim3(gr.x, gr.y - 1), dim3(TS), 0, st>>>(k);
            k_pair_row_seq<PRS, TS, true><<<dim3(gr.x, 1u), dim3(TS), 0, st>>>(k);
        }
        plan_note(" R:pair_row_seq");
    } else if (k.p.htab) {
        if constexpr (N2 <= 8192) k_pair_row<PR, TR, false, true><<<gr, dim3(TR), 0, st>>>(k);
        plan_note(" R:pair_row_htab");
    } else if (k.p.tail_a) {
        if constexpr (N2 <= 8192) k_pair_row<PR, TR, true><<<gr, dim3(TR), 0, st>>>(k);
        plan_note(" R:pair_row_tail");
    } else {
        if constexpr (N2 < 8192) k_pair_row<PR, TR><<<gr, dim3(TR), 0, st>>>(k);
        plan_note(" R:pair_row");
    }
    tk_end(st);
    LAUNCHCHK();

    const bool fast = PC::kItemsExact && fast_epilogue(k);
    // the fast pass C on 1024-point columns nulls the always-nulled samples
    // itself (PairCols::passC_fast32<true>) and leaves the fix-up the
    // f-dependent positions
    const bool nullc = fast && N1 == 1024 && S::kMaskTable && k.mtab;
    // the generic pass C reads the null decisions as bits, the nulling one
    // the table's always bits (built beside pass A or the row pass: long done)
    if (k.mask_ready && (!fast || nullc)) HIPCHK(hipStreamWaitEvent(st, k.mask_ready, 0));
    tk_begin(TK_COLC, st);
    if (fast) {
        const dim3 g16((unsigned)(N2 / 16), (unsigned)k.npairs);
        if constexpr (N1 == 2048) {
            k_pairC_fast32<typename S::PCFast32, 512><<<g16, dim3(512), 0, st>>>(k);
            plan_note(" C:fast32");
        } else if constexpr (N1 == 1024) {
            if (nullc) k_pairC_null<typename S::PCFast32><<<g16, dim3(512), 0, st>>>(k);
            else k_pairC_fast32<typename S::PCFast32, 512, 4><<<g16, dim3(512), 0, st>>>(k);
            plan_note(nullc ? " C:fast C:cols16x2 C:null" : " C:fast C:cols16x2");
        } else if constexpr (PC::kItemsExact) {
            k_pairC_fast<typename S::PCFast, T><<<gc, dim3(T), 0, st>>>(k);
            plan_note(" C:fast");
        }
    } else if (PC::kRegCols && fold_epilogue(k)) {
        if constexpr (PC::kRegCols) {
            constexpr int FB = S::FB;
            k_pairC_fold<typename S::PCFold, FB><<<dim3((unsigned)(N2 / FB), gc.y), dim3(FB), 0, st>>>(k);
        }
        plan_note(" C:fold");
    } else {
        k_pairC<PC, T><<<gc, dim3(T), 0, st>>>(k);
        plan_note(" C:generic");
    }
    tk_end(st);
    LAUNCHCHK();

    if (fast && k.mtab) {
        if (k.mask_ready && !nullc) HIPCHK(hipStreamWaitEvent(st, k.mask_ready, 0));
        KP kf = k;
        if (nullc) {   // the f-dependent words' list in place of the full one
            kf.wlist = reinterpret_cast<const uint32_t *>(w + L.wlist_f);
            kf.nwlist = reinterpret_cast<const uint32_t *>(w + L.wcount_f);
        }
        if (const int rc = launch_null_fix(kf, st, nullc)) return rc;
        plan_note(" N:fix_list");
    }
    return PSS_OK;
}

// Mixed-radix four-step (see smooth_split): columns of N1 in registers (one
// column per thread, B = T columns per workgroup) on the row engine of k.N2.
// Generic (looped) column kernels; no mask table.
template <int N1, typename CF, typename CI, int T>
static int launch_smooth_n2(KP &k, hipStream_t st) {
    using C = RegCols<N1, CF, CI, T>;
    switch (k.N2) {
        case 1024: return launch_pair<Split<C, RowsOf<1024>>>(k, st, nullptr);
        case 2048: return launch_pair<Split<C, RowsOf<2048>>>(k, st, nullptr);
        case 4096: return launch_pair<Split<C, RowsOf<4096>>>(k, st, nullptr);
        case 8192: return launch_pair<Split<C, RowsOf<8192>>>(k, st, nullptr);
        default: return fail(PSS_EUNSUPPORTED, "mixed-radix four-step: N2=%lld", (long long)k.N2);
    }
}
