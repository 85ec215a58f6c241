#pragma once
// pss_toa.hpp -- the device code the two arrival-time units share: pss_toa.hip
// (FFTFIT of every profile on its own, pss_toa_fit) and pss_toa_wide.hip (one
// phase and one DM per sub-integration, pss_toa_wide_fit).  Both run the same
// front half -- load, forward transform, cross-spectrum with the template --
// and differ in what follows: WIDE = false goes on to the coarse maximum and
// the refinement of the profile; WIDE = true writes X_k, k = 1 .. K, and the
// profile's sums to the workspace and ends.
//
//   k_toa_fft<Toa<M, BATCH, T, ...>, VEC, WIDE> : nbin = 2 M = 2^m, 32 <= nbin <= 4096.
//       A workgroup owns BATCH consecutive profiles.  A profile is ONE complex
//       sequence of M points, z[n] = p[2n] + i p[2n + 1], on the Stockham engine
//       of pss_fft.hpp, so that no bit of a profile's result depends on the
//       profiles beside it (two profiles packed as real and imaginary part of
//       one transform round each other's spectra differently, and a NaN in one
//       reaches the other).
//         load    : 16-B (VEC) or element loads -> LDS, natural order; a
//                   non-finite sample flags its profile;
//         FFT     : registers + one LDS exchange per stage;
//         split   : a group of G = min(64, M / 16) lanes owns a profile, lanes
//                   along k.  The mirror read Z[k], Z[M - k] gives P_k and
//                   P_{M-k}; they are multiplied by the conjugate template of
//                   the profile's own channel, sum |P_k|^2 and sum |S_k|^2 are
//                   accumulated per lane and reduced by xor exchanges (a fixed
//                   order), the cross-spectrum X goes to a second LDS buffer
//                   and, folded back into a half-length sequence, in place of
//                   Z;
//         inverse : the same engine; the M complex results are the N values
//                   of the coarse correlation function, even and odd lags;
//         refine  : the group finds the first maximum (value, then the lower
//                   index), then runs the safeguarded Newton iteration on
//                   delta with X read from LDS, and its first lane writes the
//                   row of out.
//   k_toa_direct<VEC, WIDE> : every other nbin in [8, 8192].  A workgroup owns one
//       profile: the twiddle table e^{-2 pi i m / nbin}, m <= nbin / 2, in
//       float64 (the other half by symmetry), the profile and X live in LDS;
//       thread t sums the harmonics t, t + 256, ... in float64 (gfx950 issues
//       float64 FMAs at half the float32 rate; the loop is bound by its LDS
//       reads) and then the lags t, t + 256, ... of the coarse grid, the phase
//       (k n) mod nbin kept by adding and wrapping; wave 0 runs the same
//       refinement.  O(K nbin) per profile.
//   Same bits whatever the alignment (the loads alone differ), the strides,
//   the number of profiles and the run.  No atomics; no workspace but the one
//   WIDE writes its results to.
#include "pss_common.hpp"
#include "pss_fft.hpp"

using namespace pss;

static constexpr int kToaIters = 24;                       // Newton / bisection steps before status 1
static constexpr float kToaTol = 1.4901161193847656e-08f;  // 2^-26 turns
static constexpr float kTwoPi = 6.283185307179586f;
static constexpr int kDirThreads = 256;

struct ToaArgs {
    const float *data, *tspec;
    float *out;
    int64_t ld, out_ld, nprof;
    int32_t nsub, nbin, K, per_chan;
    // WIDE: the workspace, sub-integration-major -- X [nsub][nchan][K] and the
    // sums [nsub][nchan][kWideMeta]
    cf *wx;
    double *wmeta;
    int32_t nchan;
};

// the sums of a profile in the workspace of the wideband fit: sum |P_k|^2,
// sum |S_k|^2, sum k^2 |S_k|^2, P_0, and 1 for a profile with a non-finite sample
static constexpr int kWideMeta = 5;

__device__ __forceinline__ void toa_wide_meta(const ToaArgs &a, int64_t chan, int64_t sub, double pp, double s2,
                                              double t2, float P0, bool bad) {
    double *m = a.wmeta + (sub * a.nchan + chan) * kWideMeta;
    m[0] = pp; m[1] = s2; m[2] = t2; m[3] = (double)P0; m[4] = bad ? 1.0 : 0.0;
}

template <bool VEC>
__device__ __forceinline__ void toa_ld4(const float *p, float (&v)[4]) {
    if (VEC) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = p[i];
    }
}

__device__ __forceinline__ bool toa_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// sums and the first maximum over the G lanes of a group (G a power of two
// <= 64, groups aligned in the wave): xor exchanges, every lane ends with the
// same bits
template <int G, typename V>
__device__ __forceinline__ V gsum(V v) {
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
template <int G>
__device__ __forceinline__ void gargmax(float &v, int &j) {
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(v, m, 64);
        const int oj = __shfl_xor(j, m, 64);
        if (ov > v || (ov == v && oj < j)) {
            v = ov;
            j = oj;
        }
    }
}

struct ToaFit {
    double C;               // float64 sum of the float32 terms: R differences it with sum |P_k|^2
    float delta, D;
    int status;
};

// The root of C' in [-1/N, 1/N] around the coarse maximum jstar, by Newton
// steps on delta kept inside the bracket that the sign of C' maintains.  The
// phase of harmonic k is ((k jstar) mod N) / N, exact in integers, plus
// k delta: X_k is turned by the first part once (xput stores it back; the lane
// that reads X_k is the one that wrote it), so that an evaluation takes the
// sine of the small angle k delta alone, |k delta| < 1/2 -- next to the root
// every term of C' is then small, not a difference of large ones, and the
// steps fall below 2^-26 turns with one harmonic as with many.  xat(k) is X_k.
// Every lane of the wave calls it (`live` false: a group without a profile).
template <int G, typename XAt, typename XPut>
__device__ __forceinline__ ToaFit toa_refine(XAt xat, XPut xput, int K, int jstar, int N, int gl, bool live) {
    const float fN = (float)N;
    float lo = -1.0f / fN, hi = 1.0f / fN, d = 0.0f;
    ToaFit f;
    f.delta = 0.0f; f.C = 0.0; f.D = 0.0f; f.status = 1;
    bool done = !live;
    const uint32_t uN = (uint32_t)N;
    {
        uint32_t m = ((uint32_t)(1 + gl) * (uint32_t)jstar) % uN;
        const uint32_t dm = ((uint32_t)G * (uint32_t)jstar) % uN;
        for (int k = 1 + gl; k <= K; k += G) {
            float r = (float)m / fN;
            if (r > 0.5f) r -= 1.0f;
            cf e;
            sincospif(2.0f * r, &e.y, &e.x);
            xput(k, cmul(xat(k), e));
            m += dm;
            if (m >= uN) m -= uN;
        }
    }
    for (int it = 0; it < kToaIters; ++it) {
        double c = 0.0;
        float g = 0.0f, dd = 0.0f;
        for (int k = 1 + gl; k <= K; k += G) {
            const cf x = xat(k);
            const float kf = (float)k;
            // (sincospi, not the native sine: with few harmonics its 1.2e-7 would be the fit's error)
            cf e;
            sincospif(2.0f * (kf * d), &e.y, &e.x);
            const float re = fmaf(x.x, e.x, -(x.y * e.y));
            const float im = fmaf(x.x, e.y, x.y * e.x);
            c += (double)re;
            g = fmaf(kf, im, g);
            dd = fmaf(kf * kf, re, dd);
        }
        c = gsum<G>(c);
        g = gsum<G>(g);
        dd = gsum<G>(dd);
        if (!done) {
            f.delta = d; f.C = c; f.D = dd;
            if (g == 0.0f) {
                f.status = 0;
                done = true;
            } else {
                // C' = -2 pi g, C'' = -4 pi^2 D
                if (g < 0.0f) lo = d; else hi = d;
                // (a Newton step below the tolerance ends the iteration before the
                // bracket is asked: at the root d is itself an end of the bracket)
                float dn = d - g / (kTwoPi * dd);
                const bool small = dd > 0.0f && fabsf(dn - d) < kToaTol;
                if (!small && (!(dd > 0.0f) || !(dn > lo && dn < hi))) dn = 0.5f * (lo + hi);
                if (fabsf(dn - d) < kToaTol) {
                    f.status = 0;
                    done = true;
                } else {
                    d = dn;
                }
            }
        }
        if (__builtin_amdgcn_ballot_w64(!done) == 0) break;
    }
    return f;
}

// the row of out from the sums of one profile (PP, S2 and C are float64 sums of
// float32 terms, R their difference in float64, rounded once)
__device__ __forceinline__ void toa_write(float *o, int N, int K, int jstar, ToaFit f, double PP, double S2d, float P0,
                                          float S0, bool bad) {
    const float inf = __builtin_huge_valf();
    const float nan = __uint_as_float(0x7FC00000u);
    float tau, tau_err, b, b_err, a, rms, snr, status;
    if (bad) {
        tau = 0.0f; tau_err = inf; b_err = inf; b = nan; a = nan; rms = nan; snr = nan; status = 2.0f;
    } else {
        const float fN = (float)N;
        const float C = (float)f.C, S2 = (float)S2d;
        const bool degen = !(C > 0.0f) || !(f.D > 0.0f);
        const int jw = 2 * jstar >= N ? jstar - N : jstar;
        tau = (float)jw / fN + (degen ? 0.0f : f.delta);
        if (tau >= 0.5f) tau -= 1.0f;
        if (tau < -0.5f) tau += 1.0f;
        b = (float)(f.C / S2d);
        a = (P0 - b * S0) / fN;
        const float R = (float)(PP - f.C * f.C / S2d);
        const float sig2 = K > 1 ? fmaxf(R, 0.0f) / (float)(2 * K - 2) : inf;
        tau_err = degen ? inf : sqrtf(sig2 / (b * f.D)) / kTwoPi;
        b_err = degen ? inf : sqrtf(sig2 / S2);
        rms = sqrtf(2.0f * sig2 / fN);
        snr = b / b_err;
        status = degen ? 2.0f : (float)f.status;
    }
    o[0] = tau; o[1] = tau_err; o[2] = b; o[3] = b_err; o[4] = a; o[5] = rms; o[6] = snr; o[7] = status;
}

// ---------------------------------------------------------------------------
// FFT path
// ---------------------------------------------------------------------------
template <int M_, int BATCH_, int T_, typename F>
struct Toa;

template <int M_, int BATCH_, int T_, int... F>
struct Toa<M_, BATCH_, T_, RList<F...>> {
    static constexpr int M = M_, N = 2 * M_, BATCH = BATCH_, T = T_;
    using FF = Fft<M, BATCH, T>;                            // the inverse: an argmax follows it
    using FP = Fft<M, BATCH, T, false, 1, true>;            // forward: sincospi twiddles (R differences its powers)
    using LD = Lds<M>;
    static constexpr int E = FF::E;
    static constexpr int RF0 = FF::template first<F...>();
    static constexpr int RFL = FF::template last_of<F...>();
    static constexpr int G = M / 16 < 64 ? M / 16 : 64;     // lanes of a profile's group
    static_assert(T / G >= BATCH, "every profile of the workgroup needs a group");

    template <bool VEC, bool WIDE>
    __device__ static void body(const ToaArgs &a) {
        __shared__ __align__(16) cf lds[BATCH * LD::RS];    // Z, then the folded cross-spectrum, then C
        __shared__ __align__(16) cf xs[BATCH * LD::RS];     // X_k, k < M (0 above K)
        __shared__ int bad[BATCH];
        const int tid = threadIdx.x;
        const int64_t r0 = (int64_t)xcd_run_id() * BATCH;
        const int K = a.K;
        for (int i = tid; i < BATCH; i += T) bad[i] = 0;
        __syncthreads();
        // ---- load
        for (int it = tid; it < BATCH * (N / 4); it += T) {
            const int b = it / (N / 4);
            const int j = (it - b * (N / 4)) * 4;
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            const int64_t r = r0 + b;
            if (r < a.nprof) {
                const int64_t c = r / a.nsub, s = r - c * a.nsub;
                const float *src = a.data + c * a.ld + s * (int64_t)N;
                toa_ld4<VEC>(src + j, v);
                if (!(toa_finite(v[0]) && toa_finite(v[1]) && toa_finite(v[2]) && toa_finite(v[3]))) bad[b] = 1;
                // (the profile's first sample is taken off: the harmonics k >= 1 do not see it; P_0 gets it back)
                const float p0 = src[0];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] -= p0;
            }
            lds[LD::at(b, j / 2)] = make_float2(v[0], v[1]);
            lds[LD::at(b, j / 2 + 1)] = make_float2(v[2], v[3]);
        }
        __syncthreads();
        {
            cf v[E];
            FP::template load<RF0>(v, lds, tid);
            __syncthreads();
            FP::template run<false, 1, F...>(v, lds, tid);
            FP::template store<RFL>(v, lds, tid);
        }
        __syncthreads();
        // ---- split, cross-spectrum, fold
        const int gid = tid / G, gl = tid - gid * G;
        const bool own = gid < BATCH;
        const int b = own ? gid : 0;
        const int64_t r = r0 + b;
        const bool valid = own && r < a.nprof;
        const int64_t chan = valid ? r / a.nsub : 0;
        const float *tp = a.tspec + (a.per_chan ? chan : 0) * (int64_t)(K + 1) * 2;
        float P0 = 0.0f;
        double pp = 0.0, s2 = 0.0, t2 = 0.0;
        if (own) {
            for (int k = gl; k <= M / 2; k += G) {
                const int k2 = (M - k) & (M - 1);
                const cf za = lds[LD::at(b, k)];
                if (k == 0) {
                    P0 = fmaf((float)N, valid ? a.data[chan * a.ld + (r - chan * a.nsub) * (int64_t)N] : 0.0f, za.x + za.y);
                    lds[LD::at(b, 0)] = make_float2(0.0f, 0.0f);
                    xs[LD::at(b, 0)] = make_float2(0.0f, 0.0f);
                    continue;
                }
                const cf zb = lds[LD::at(b, k2)];
                cf w;                                                     // e^{-2 pi i k / N}
                sincospif(-(float)k / (float)M, &w.y, &w.x);
                const cf A = make_float2(za.x + zb.x, za.y - zb.y);
                const cf B = make_float2(za.x - zb.x, za.y + zb.y);
                const cf t = cmul(w, B);
                const cf pk = make_float2(0.5f * (A.x + t.y), 0.5f * (A.y - t.x));
                const cf pk2 = make_float2(0.5f * (A.x - t.y), 0.5f * (-A.y - t.x));
                cf yk = make_float2(0.0f, 0.0f), yk2 = make_float2(0.0f, 0.0f);
                if (k <= K) {
                    const cf s = make_float2(tp[2 * k], tp[2 * k + 1]);
                    yk = cmul_conj(pk, s);
                    pp += (double)fmaf(pk.x, pk.x, pk.y * pk.y);
                    s2 += (double)fmaf(s.x, s.x, s.y * s.y);
                    if constexpr (WIDE) t2 += (double)k * (double)k * (double)fmaf(s.x, s.x, s.y * s.y);
                }
                if (k2 <= K && k2 != k) {
                    const cf s = make_float2(tp[2 * k2], tp[2 * k2 + 1]);
                    yk2 = cmul_conj(pk2, s);
                    pp += (double)fmaf(pk2.x, pk2.x, pk2.y * pk2.y);
                    s2 += (double)fmaf(s.x, s.x, s.y * s.y);
                    if constexpr (WIDE) t2 += (double)k2 * (double)k2 * (double)fmaf(s.x, s.x, s.y * s.y);
                }
                if (k2 == k) yk2 = yk;
                xs[LD::at(b, k)] = yk;
                xs[LD::at(b, k2)] = yk2;
                // V_k = (Y_k + conj Y_k2) + i conj(w) (Y_k - conj Y_k2), V_k2 its mirror
                const cf A2 = make_float2(yk.x + yk2.x, yk.y - yk2.y);
                const cf B2 = make_float2(yk.x - yk2.x, yk.y + yk2.y);
                const cf t2 = cmul_conj(B2, w);
                lds[LD::at(b, k)] = make_float2(A2.x - t2.y, A2.y + t2.x);
                lds[LD::at(b, k2)] = make_float2(A2.x + t2.y, t2.x - A2.y);
            }
        }
        pp = gsum<G>(pp);
        s2 = gsum<G>(s2);
        P0 = gsum<G>(P0);                                   // (lane 0 of the group holds it, the others 0)
        __syncthreads();
        if constexpr (WIDE) {
            // ---- the wideband fit takes over from here: X_k, k = 1 .. K, and the sums
            t2 = gsum<G>(t2);
            if (valid) {
                const int64_t sub = r - chan * a.nsub;
                cf *dst = a.wx + (sub * a.nchan + chan) * (int64_t)K;
                for (int k = 1 + gl; k <= K; k += G) dst[k - 1] = xs[LD::at(b, k)];
                if (gl == 0) toa_wide_meta(a, chan, sub, pp, s2, t2, P0, bad[b] != 0);
            }
            return;
        }
        {
            cf v[E];
            FF::template load<RF0>(v, lds, tid);
            __syncthreads();
            FF::template run<true, 1, F...>(v, lds, tid);
            FF::template store<RFL>(v, lds, tid);
        }
        __syncthreads();
        // ---- first maximum of C_j, j = 2 p and 2 p + 1 at position p
        float best = -__builtin_huge_valf();
        int jstar = 0;
        if (own) {
            for (int p = gl; p < M; p += G) {
                const cf c = lds[LD::at(b, p)];
                if (c.x > best) { best = c.x; jstar = 2 * p; }
                if (c.y > best) { best = c.y; jstar = 2 * p + 1; }
            }
        }
        gargmax<G>(best, jstar);
        const bool isbad = valid && bad[b] != 0;
        cf *xb = xs;
        const ToaFit f = toa_refine<G>([xb, b](int k) { return xb[LD::at(b, k)]; },
                                       [xb, b, own](int k, cf v) { if (own) xb[LD::at(b, k)] = v; }, K, jstar, N, gl,
                                       valid && !isbad);
        if (valid && gl == 0) toa_write(a.out + r * a.out_ld, N, K, jstar, f, pp, s2, P0, tp[0], isbad);
    }
};

template <typename TT, bool VEC, bool WIDE>
__global__ __launch_bounds__(TT::T) void k_toa_fft(ToaArgs a) { TT::template body<VEC, WIDE>(a); }

template <typename TT, bool WIDE>
static int launch_toa_fft(const char *what, const ToaArgs &a, bool vec, hipStream_t st) {
    const int64_t ngroups = (a.nprof - 1) / TT::BATCH + 1;
    if (ngroups > 0x7fffffff)
        return fail(PSS_EINVAL, "%s: %lld workgroups exceed 2^31 - 1", what, (long long)ngroups);
    if (vec) k_toa_fft<TT, true, WIDE><<<dim3((unsigned)ngroups), dim3(TT::T), 0, st>>>(a);
    else k_toa_fft<TT, false, WIDE><<<dim3((unsigned)ngroups), dim3(TT::T), 0, st>>>(a);
    LAUNCHCHK();
    return PSS_OK;
}

// ---------------------------------------------------------------------------
// direct path
// ---------------------------------------------------------------------------
template <bool VEC, bool WIDE>
__global__ __launch_bounds__(kDirThreads) void k_toa_direct(ToaArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ double redf[WIDE ? 3 : 2][kDirThreads / 64];
    __shared__ int redi[kDirThreads / 64];
    __shared__ int bad;
    const int N = a.nbin, K = a.K;
    const int h = N / 2;
    double2 *tw = reinterpret_cast<double2 *>(smem);        // [h + 1]: e^{-2 pi i m / N}, m <= N / 2
    cf *xs = reinterpret_cast<cf *>(tw + h + 1);            // [K + 1]: xs[0] = (P_0, 0)
    float *pf = reinterpret_cast<float *>(xs + K + 1);      // [N]
    const int tid = threadIdx.x;
    const int64_t r = xcd_run_id();
    const int64_t chan = r / a.nsub, sub = r - chan * a.nsub;
    const float *src = a.data + chan * a.ld + sub * (int64_t)N;
    const float *tp = a.tspec + (a.per_chan ? chan : 0) * (int64_t)(K + 1) * 2;
    if (tid == 0) bad = 0;
    for (int m = tid; m <= h; m += kDirThreads) {
        double s, c;
        sincospi(-2.0 * (double)m / (double)N, &s, &c);
        tw[m] = make_double2(c, s);
    }
    __syncthreads();
    bool nf = false;
    if (VEC) {
        for (int j = 4 * tid; j < N; j += 4 * kDirThreads) {
            float v[4];
            toa_ld4<true>(src + j, v);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                pf[j + i] = v[i];
                nf = nf || !toa_finite(v[i]);
            }
        }
    } else {
        for (int j = tid; j < N; j += kDirThreads) {
            const float v = src[j];
            pf[j] = v;
            nf = nf || !toa_finite(v);
        }
    }
    if (nf) bad = 1;
    __syncthreads();
    // ---- harmonics tid, tid + 256, ...: float64 sums of the float32 samples
    // (a harmonic where the template's components nearly cancel is small next
    // to the sum of |p|; float32 twiddles alone would cost it 1e-6), rounded
    // once.  The first sample is taken off, exactly, before the sums: the
    // harmonics k >= 1 do not see it, a constant profile gives exact zeros,
    // and P_0 gets it back.
    const double p0 = (double)pf[0];
    double pp = 0.0, s2 = 0.0, t2 = 0.0;
    for (int k = tid; k <= K; k += kDirThreads) {
        double re = 0.0, im = 0.0;
        int m = 0;
        for (int n = 0; n < N; ++n) {
            const double2 t = tw[m <= h ? m : N - m];
            const double p = (double)pf[n] - p0;
            re = fma(p, t.x, re);
            im = fma(p, m <= h ? t.y : -t.y, im);
            m += k;
            if (m >= N) m -= N;
        }
        if (k == 0) {
            xs[0] = make_float2((float)fma((double)N, p0, re), 0.0f);
        } else {
            const cf pk = make_float2((float)re, (float)im);
            const cf s = make_float2(tp[2 * k], tp[2 * k + 1]);
            xs[k] = cmul_conj(pk, s);
            pp += (double)fmaf(pk.x, pk.x, pk.y * pk.y);
            s2 += (double)fmaf(s.x, s.x, s.y * s.y);
            if constexpr (WIDE) t2 += (double)k * (double)k * (double)fmaf(s.x, s.x, s.y * s.y);
        }
    }
    pp = gsum<64>(pp);
    s2 = gsum<64>(s2);
    if constexpr (WIDE) t2 = gsum<64>(t2);
    if ((tid & 63) == 0) {
        redf[0][tid >> 6] = pp;
        redf[1][tid >> 6] = s2;
        if constexpr (WIDE) redf[2][tid >> 6] = t2;
    }
    __syncthreads();
    pp = 0.0;
    s2 = 0.0;
#pragma unroll
    for (int w = 0; w < kDirThreads / 64; ++w) {
        pp += redf[0][w];
        s2 += redf[1][w];
    }
    if constexpr (WIDE) {
        // ---- the wideband fit takes over from here: X_k, k = 1 .. K, and the sums
        t2 = 0.0;
#pragma unroll
        for (int w = 0; w < kDirThreads / 64; ++w) t2 += redf[2][w];
        cf *dst = a.wx + (sub * a.nchan + chan) * (int64_t)K;
        for (int k = 1 + tid; k <= K; k += kDirThreads) dst[k - 1] = xs[k];
        if (tid == 0) toa_wide_meta(a, chan, sub, pp, s2, t2, xs[0].x, bad != 0);
        return;
    }
    // ---- lags tid, tid + 256, ... of the coarse grid
    float best = -__builtin_huge_valf();
    int jstar = 0;
    for (int j = tid; j < N; j += kDirThreads) {
        double c = 0.0;
        int m = j;
        for (int k = 1; k <= K; ++k) {
            const cf x = xs[k];
            const double2 t = tw[m <= h ? m : N - m];
            c = fma((double)x.x, t.x, c);
            c = fma((double)x.y, m <= h ? t.y : -t.y, c);
            m += j;
            if (m >= N) m -= N;
        }
        const float cj = (float)c;
        if (cj > best) { best = cj; jstar = j; }
    }
    gargmax<64>(best, jstar);
    __syncthreads();                                         // (redf is read above)
    if ((tid & 63) == 0) {
        redf[0][tid >> 6] = (double)best;
        redi[tid >> 6] = jstar;
    }
    __syncthreads();
    if (tid < 64) {
        best = (float)redf[0][0];
        jstar = redi[0];
#pragma unroll
        for (int w = 1; w < kDirThreads / 64; ++w) {
            const float ov = (float)redf[0][w];
            const int oj = redi[w];
            if (ov > best || (ov == best && oj < jstar)) { best = ov; jstar = oj; }
        }
        const bool isbad = bad != 0;
        cf *xb = xs;
        const ToaFit f = toa_refine<64>([xb](int k) { return xb[k]; }, [xb](int k, cf v) { xb[k] = v; }, K, jstar, N,
                                        tid, !isbad);
        if (tid == 0) toa_write(a.out + r * a.out_ld, N, K, jstar, f, pp, s2, xs[0].x, tp[0], isbad);
    }
}

// the dynamic LDS of k_toa_direct
static inline size_t toa_direct_lds(int nbin, int K) {
    return (size_t)(nbin / 2 + 1) * 16 + (size_t)(K + 1) * 8 + (size_t)nbin * 4;
}

// The front half (WIDE) or the whole fit of a.nprof profiles: nbin = 2^m in
// [32, 4096] on the FFT path, every other length by the direct sums.
template <bool WIDE>
static int launch_toa(const char *what, const ToaArgs &a, bool vec, hipStream_t st) {
    switch (a.nbin) {
        case 32: return launch_toa_fft<Toa<16, 256, 256, C16>, WIDE>(what, a, vec, st);
        case 64: return launch_toa_fft<Toa<32, 128, 256, C32F>, WIDE>(what, a, vec, st);
        case 128: return launch_toa_fft<Toa<64, 64, 256, C64F>, WIDE>(what, a, vec, st);
        case 256: return launch_toa_fft<Toa<128, 32, 256, C128F>, WIDE>(what, a, vec, st);
        case 512: return launch_toa_fft<Toa<256, 16, 256, C256>, WIDE>(what, a, vec, st);
        case 1024: return launch_toa_fft<Toa<512, 8, 256, C512F>, WIDE>(what, a, vec, st);
        case 2048: return launch_toa_fft<Toa<1024, 4, 256, C1kF>, WIDE>(what, a, vec, st);
        case 4096: return launch_toa_fft<Toa<2048, 2, 256, C2kF>, WIDE>(what, a, vec, st);
        default: break;
    }
    if (a.nprof > 0x7fffffff)
        return fail(PSS_EINVAL, "%s: %lld workgroups exceed 2^31 - 1", what, (long long)a.nprof);
    const size_t bytes = toa_direct_lds(a.nbin, a.K);
    if (bytes > 65536) {                                     // (dynamic LDS above 64 KB has to be asked for)
        const void *fn = vec ? reinterpret_cast<const void *>(k_toa_direct<true, WIDE>)
                             : reinterpret_cast<const void *>(k_toa_direct<false, WIDE>);
        HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    }
    if (vec) k_toa_direct<true, WIDE><<<dim3((unsigned)a.nprof), dim3(kDirThreads), bytes, st>>>(a);
    else k_toa_direct<false, WIDE><<<dim3((unsigned)a.nprof), dim3(kDirThreads), bytes, st>>>(a);
    LAUNCHCHK();
    return PSS_OK;
}
