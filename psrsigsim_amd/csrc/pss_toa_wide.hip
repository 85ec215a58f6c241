// pss_toa_wide.hip -- wideband arrival times (extension, no reference
// counterpart): one phase and one DM per sub-integration, fitted to all the
// channels of the sub-integration at once (Pennucci, Demorest & Ransom 2014);
// include/pss_hip.h has the definitions.  Nine kinds of launch, nothing read
// back in between:
//
//   spectrum : the front half of pss_toa_fit (pss_toa.hpp, WIDE): X_nk, k = 1 ..
//       K, as float2 to the workspace, sub-integration-major, and per profile
//       sum |P_k|^2, sum |S_k|^2, sum k^2 |S_k|^2, P_0 and the bad flag.
//   k_wide_list : one wave per sub-integration.  The usable channels (weight
//       finite and > 0, no non-finite sample) in index order, by ballots; every
//       later stage walks this list, so that a channel that is left out leaves
//       the bits of the fit what they are without it.  kappa's mean and span
//       over the list; the rows of prof of the channels left out.
//   k_wide_xbar : a wave per (sub-integration, DM trial, 64 harmonics).  A
//       lane owns a harmonic and walks the list in order: Xbar_k to the
//       workspace.  (One workgroup per trial, its threads striding over the
//       harmonics, forms the same sums in the same order on 15 CUs instead of
//       240: the start took 3.4 ms that way and takes 1.1 ms this way at 2048
//       channels x 15 sub-integrations x 2048 bins.)
//   k_wide_coarse : one workgroup per (sub-integration, DM trial): the lags t,
//       t + 256, ... by direct float64 sums over a twiddle table in LDS, as
//       k_toa_direct forms them, and the first maximum.
//   k_wide_init : the start (phi, d) of every sub-integration from its trials.
//   k_wide_eval<G, FINAL> : grid over (sub-integration, block of 256 / G list
//       entries).  A group of G lanes along k owns a channel: k phi_n in
//       float64, reduced, then sincospif; C_n, g_n, D_n are float64 sums of
//       float32 terms, reduced by gsum.  The group's first lane forms the
//       channel's terms of the gradient, the Hessian and the expected curvature
//       in float64; lanes 0 .. 8 of the workgroup add them over the block's
//       channels in order, one sum each.  FINAL evaluates at the accepted point,
//       writes the rows of prof and adds the chi^2 terms.
//   k_wide_step : a wave per sub-integration adds the partial sums in block
//       order and applies the accept / halve / Newton rule.  A finished
//       sub-integration is flagged; its evaluations return at once.
//   k_wide_finish : errors, chi^2 and the row of out.
//
//   The 32 rounds of (eval, step) are all launched.  No atomics.
#include "pss_toa.hpp"

static constexpr int kWideEvals = 32;
static constexpr double kWideTol = 1.4901161193847656e-08;   // 2^-26 turns
static constexpr double kWideClampBins = 4.0;                // the longest step, in bins of phase across the band
static constexpr int kWideT = 256;
static constexpr int kWidePart = 9;      // q, kq, h, kh, kkh, e, ke, kke, chi2
static constexpr int kWideState = 16;
// state of a sub-integration, float64 each
enum { WS_PHI, WS_D, WS_PPHI, WS_PD, WS_TPHI, WS_TD, WS_GPHI, WS_GD, WS_NEV, WS_STATUS, WS_DONE, WS_NUSED, WS_KSPAN,
       WS_KBAR };
static constexpr double kPi = 3.141592653589793;

struct WideArgs {
    const cf *x;             // [nsub][nchan][K]
    const double *meta;      // [nsub][nchan][kWideMeta]
    const double *kappa, *phi0;
    const float *wt;         // [nchan][nsub]
    int32_t *list;           // [nsub][nchan]
    cf *xbar;                // [nsub][ndm][K]
    float2 *coarse;          // [nsub][ndm]: (value, lag as an int's bits)
    double *part;            // [nsub][nblk][kWidePart]
    double *state;           // [nsub][kWideState]
    double *out;
    float *prof;
    int64_t out_ld, prof_ld;
    double dm_step;
    int32_t nchan, nsub, nbin, K, ndm, nblk, cb;
};

struct WideLayout {
    int64_t x, meta, list, xbar, coarse, part, state, total;
    int32_t K, G, cb, nblk;
};

static inline int64_t up16(int64_t v) { return (v + 15) / 16 * 16; }

static WideLayout wide_layout(int32_t nchan, int32_t nsub, int32_t nbin, int32_t nharm, int32_t ndm) {
    WideLayout w;
    w.K = nharm < (nbin - 1) / 2 ? nharm : (nbin - 1) / 2;
    w.G = w.K > 32 ? 64 : (w.K > 8 ? 16 : 4);
    w.cb = kWideT / w.G;
    w.nblk = (nchan - 1) / w.cb + 1;
    const int64_t np = (int64_t)nchan * nsub;
    w.x = 0;
    w.meta = w.x + up16(np * w.K * 8);
    w.list = w.meta + up16(np * kWideMeta * 8);
    w.xbar = w.list + up16(np * 4);
    w.coarse = w.xbar + up16((int64_t)nsub * ndm * w.K * 8);
    w.part = w.coarse + up16((int64_t)nsub * ndm * 8);
    w.state = w.part + up16((int64_t)nsub * w.nblk * kWidePart * 8);
    w.total = w.state + up16((int64_t)nsub * kWideState * 8);
    return w;
}

__device__ __forceinline__ bool wide_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// e^{2 pi i k ph}: k ph in float64, reduced to [-1/2, 1/2], rounded once
__device__ __forceinline__ cf wide_turn(int k, double ph) {
    double t = (double)k * ph;
    t -= rint(t);
    cf e;
    sincospif(2.0f * (float)t, &e.y, &e.x);
    return e;
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_wide_list(WideArgs a) {
    const int s = blockIdx.x, lane = threadIdx.x;
    const int nchan = a.nchan;
    int32_t *list = a.list + (int64_t)s * nchan;
    int nused = 0;
    double kmin = __builtin_huge_val(), kmax = -__builtin_huge_val();
    for (int c0 = 0; c0 < nchan; c0 += 64) {
        const int c = c0 + lane;
        bool ok = false;
        if (c < nchan) {
            const float w = a.wt[(int64_t)c * a.nsub + s];
            const double *m = a.meta + ((int64_t)s * nchan + c) * kWideMeta;
            const bool bad = m[4] != 0.0;
            ok = toa_finite(w) && w > 0.0f && !bad && m[1] > 0.0;
            if (!ok) {
                float *o = a.prof + ((int64_t)c * a.nsub + s) * a.prof_ld;
                o[0] = bad ? __uint_as_float(0x7FC00000u) : 0.0f;
                o[1] = __builtin_huge_valf();
                o[2] = 0.0f;
                o[3] = 0.0f;
            }
        }
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(ok);
        if (ok) {
            list[nused + __popcll(mask & ((1ull << lane) - 1ull))] = c;
            const double k = a.kappa[c];
            kmin = fmin(kmin, k);
            kmax = fmax(kmax, k);
        }
        nused += __popcll(mask);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        kmin = fmin(kmin, __shfl_xor(kmin, m, 64));
        kmax = fmax(kmax, __shfl_xor(kmax, m, 64));
    }
    __syncthreads();                                         // (the list is read back below)
    double ks = 0.0;
    for (int r = lane; r < nused; r += 64) ks += a.kappa[list[r]];
    ks = gsum<64>(ks);
    if (lane == 0) {
        double *st = a.state + (int64_t)s * kWideState;
        const double kbar = nused > 0 ? ks / (double)nused : 0.0;
        st[WS_NUSED] = (double)nused;
        st[WS_KBAR] = kbar;
        st[WS_KSPAN] = nused > 0 ? fmax(kmax - kbar, kbar - kmin) : 0.0;
    }
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_wide_xbar(WideArgs a, int nkb) {
    const int K = a.K;
    const int kb = blockIdx.x % nkb, st = blockIdx.x / nkb;  // st = s * ndm + it
    const int s = st / a.ndm, it = st - s * a.ndm;
    const int k = 1 + kb * 64 + (int)threadIdx.x;
    if (k > K) return;
    const double d = (double)(it - a.ndm / 2) * a.dm_step;
    const int nused = (int)a.state[(int64_t)s * kWideState + WS_NUSED];
    const int32_t *list = a.list + (int64_t)s * a.nchan;
    double re = 0.0, im = 0.0;
    for (int r = 0; r < nused; ++r) {
        const int n = list[r];
        double ph = a.phi0[n] + a.kappa[n] * d;
        ph -= rint(ph);
        const cf e = wide_turn(k, ph);
        const cf x = a.x[((int64_t)s * a.nchan + n) * K + (k - 1)];
        const float w = a.wt[(int64_t)n * a.nsub + s];
        re += (double)(w * fmaf(x.x, e.x, -(x.y * e.y)));
        im += (double)(w * fmaf(x.x, e.y, x.y * e.x));
    }
    a.xbar[(int64_t)st * K + (k - 1)] = make_float2((float)re, (float)im);
}

__global__ __launch_bounds__(kWideT) void k_wide_coarse(WideArgs a) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ float redv[kWideT / 64];
    __shared__ int redj[kWideT / 64];
    const int N = a.nbin, K = a.K, h = N / 2;
    double2 *tw = reinterpret_cast<double2 *>(smem);        // [h + 1]: e^{-2 pi i m / N}
    cf *xb = reinterpret_cast<cf *>(tw + h + 1);            // [K + 1]
    const int tid = threadIdx.x;
    const int s = blockIdx.x / a.ndm, it = blockIdx.x - s * a.ndm;
    for (int m = tid; m <= h; m += kWideT) {
        double sn, cs;
        sincospi(-2.0 * (double)m / (double)N, &sn, &cs);
        tw[m] = make_double2(cs, sn);
    }
    for (int k = 1 + tid; k <= K; k += kWideT) xb[k] = a.xbar[(int64_t)blockIdx.x * K + (k - 1)];
    __syncthreads();
    // ---- the lags tid, tid + 256, ...: C_j = sum_k Re[Xbar_k e^{+2 pi i k j / N}]
    float best = -__builtin_huge_valf();
    int jstar = 0;
    for (int j = tid; j < N; j += kWideT) {
        double c = 0.0;
        int m = j;
        for (int k = 1; k <= K; ++k) {
            const cf x = xb[k];
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
    if ((tid & 63) == 0) {
        redv[tid >> 6] = best;
        redj[tid >> 6] = jstar;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kWideT / 64; ++w)
            if (redv[w] > best || (redv[w] == best && redj[w] < jstar)) { best = redv[w]; jstar = redj[w]; }
        a.coarse[(int64_t)s * a.ndm + it] = make_float2(best, __int_as_float(jstar));
    }
}

// the start of every sub-integration: the trial with the largest value; ties
// to the lower |i|, then the lower i (the lag's tie is settled in its trial)
__global__ __launch_bounds__(64) void k_wide_init(WideArgs a) {
    for (int s = threadIdx.x; s < a.nsub; s += 64) {
        double *st = a.state + (int64_t)s * kWideState;
        const int half = a.ndm / 2;
        float best = 0.0f;
        int bi = 0, bj = 0;
        bool have = false;
        for (int it = 0; it < a.ndm; ++it) {
            const float2 c = a.coarse[(int64_t)s * a.ndm + it];
            const int i = it - half, ai = i < 0 ? -i : i, abi = bi < 0 ? -bi : bi;
            if (!have || c.x > best || (c.x == best && (ai < abi || (ai == abi && i < bi)))) {
                have = true;
                best = c.x;
                bi = i;
                bj = __float_as_int(c.y);
            }
        }
        const int jw = 2 * bj >= a.nbin ? bj - a.nbin : bj;
        const double phi = (double)jw / (double)a.nbin, d = (double)bi * a.dm_step;
        st[WS_PHI] = phi; st[WS_D] = d;
        st[WS_PPHI] = 0.0; st[WS_PD] = 0.0;
        st[WS_TPHI] = phi; st[WS_TD] = d;
        st[WS_GPHI] = 0.0; st[WS_GD] = 0.0;
        st[WS_NEV] = 0.0;
        // fewer than two distinct kappa: the DM is not determined
        const bool degen = st[WS_NUSED] < 2.0 || !(st[WS_KSPAN] > 0.0);
        st[WS_STATUS] = degen ? 2.0 : 1.0;
        st[WS_DONE] = degen ? 1.0 : 0.0;
    }
}

// ---------------------------------------------------------------------------
template <int G, bool FINAL>
__global__ __launch_bounds__(kWideT) void k_wide_eval(WideArgs a) {
    constexpr int CB = kWideT / G;
    __shared__ double vals[CB][kWidePart];
    const int tid = threadIdx.x;
    const int s = blockIdx.x / a.nblk, b = blockIdx.x - s * a.nblk;
    const double *st = a.state + (int64_t)s * kWideState;
    if (!FINAL && st[WS_DONE] != 0.0) return;
    const int nused = (int)st[WS_NUSED];
    const int r0 = b * CB;
    if (r0 >= nused) return;
    const int cnt = nused - r0 < CB ? nused - r0 : CB;
    const double phi = FINAL ? st[WS_PHI] : st[WS_TPHI], d = FINAL ? st[WS_D] : st[WS_TD];
    const int g = tid / G, gl = tid - g * G;
    const bool live = g < cnt;
    const int n = live ? a.list[(int64_t)s * a.nchan + r0 + g] : 0;
    const int K = a.K;
    double c = 0.0, gg = 0.0, dd = 0.0;
    if (live) {
        const double kap = a.kappa[n];
        double ph = a.phi0[n] + phi + kap * d;
        ph -= rint(ph);
        const cf *x = a.x + ((int64_t)s * a.nchan + n) * K;
        for (int k = 1 + gl; k <= K; k += G) {
            const cf xk = x[k - 1];
            const cf e = wide_turn(k, ph);
            const float kf = (float)k;
            const float re = fmaf(xk.x, e.x, -(xk.y * e.y));
            const float im = fmaf(xk.x, e.y, xk.y * e.x);
            c += (double)re;
            gg += (double)(kf * im);
            dd += (double)(kf * kf * re);
        }
    }
    c = gsum<G>(c);
    gg = gsum<G>(gg);
    dd = gsum<G>(dd);
    if (live && gl == 0) {
        const double kap = a.kappa[n];
        const double *m = a.meta + ((int64_t)s * a.nchan + n) * kWideMeta;
        const double wtn = (double)a.wt[(int64_t)n * a.nsub + s];
        const double PP = m[0], S2 = m[1], T2 = m[2];
        const double w = wtn / S2;
        const double c1 = -2.0 * kPi * gg, c2 = -4.0 * kPi * kPi * dd;
        const double q = 2.0 * w * c * c1;
        const double hh = 2.0 * w * (c1 * c1 + c * c2);
        const double e = -8.0 * kPi * kPi * w * c * c * (T2 / S2);
        const double chi = wtn * (PP - c * c / S2);
        double *v = vals[g];
        v[0] = q; v[1] = kap * q;
        v[2] = hh; v[3] = kap * hh; v[4] = kap * kap * hh;
        v[5] = e; v[6] = kap * e; v[7] = kap * kap * e;
        v[8] = chi;
        if (FINAL) {
            float *o = a.prof + ((int64_t)n * a.nsub + s) * a.prof_ld;
            o[0] = (float)(c / S2);
            o[1] = (float)sqrt(1.0 / (wtn * S2));
            o[2] = (float)chi;
            o[3] = 1.0f;
        }
    }
    __syncthreads();
    if (tid < kWidePart) {
        double sum = 0.0;
        for (int j = 0; j < cnt; ++j) sum += vals[j][tid];
        a.part[((int64_t)s * a.nblk + b) * kWidePart + tid] = sum;
    }
}

// lanes 0 .. 8 add one partial sum each over the blocks that hold list entries, in order
__device__ __forceinline__ void wide_reduce(const WideArgs &a, int s, int nused, double *sums) {
    const int lane = threadIdx.x;
    if (lane < kWidePart) {
        const int nb = (nused + a.cb - 1) / a.cb;
        const double *p = a.part + (int64_t)s * a.nblk * kWidePart + lane;
        double sum = 0.0;
        for (int b = 0; b < nb; ++b) sum += p[(int64_t)b * kWidePart];
        sums[lane] = sum;
    }
    __syncthreads();
}

// the Newton step -H^-1 g on the true Hessian where it is negative definite,
// on the expected curvature elsewhere; neither: no step
__device__ __forceinline__ void wide_newton(const double *S, double kspan, int nbin, double &pp, double &pd) {
    double h11 = S[2], h12 = S[3], h22 = S[4];
    double det = h11 * h22 - h12 * h12;
    if (!(h11 < 0.0 && det > 0.0)) {
        h11 = S[5]; h12 = S[6]; h22 = S[7];
        det = h11 * h22 - h12 * h12;
    }
    pp = 0.0; pd = 0.0;
    if (h11 < 0.0 && det > 0.0) {
        pp = -(h22 * S[0] - h12 * S[1]) / det;
        pd = -(h11 * S[1] - h12 * S[0]) / det;
        const double len = fmax(fabs(pp), fabs(pd) * kspan) * (double)nbin / kWideClampBins;
        if (len > 1.0) { pp /= len; pd /= len; }
        if (!(wide_finite(pp) && wide_finite(pd))) { pp = 0.0; pd = 0.0; }
    }
}

__global__ __launch_bounds__(64) void k_wide_step(WideArgs a) {
    __shared__ double S[kWidePart];
    const int s = blockIdx.x;
    double *st = a.state + (int64_t)s * kWideState;
    if (st[WS_DONE] != 0.0) return;
    wide_reduce(a, s, (int)st[WS_NUSED], S);
    if (threadIdx.x != 0) return;
    const int nev = (int)st[WS_NEV] + 1;
    double pp = st[WS_PPHI], pd = st[WS_PD];
    const double kspan = st[WS_KSPAN];
    // accept the trial point when the slope along the step has not grown
    const bool accept = nev == 1 || fabs(S[0] * pp + S[1] * pd) <= fabs(st[WS_GPHI] * pp + st[WS_GD] * pd);
    if (accept) {
        st[WS_PHI] = st[WS_TPHI]; st[WS_D] = st[WS_TD];
        st[WS_GPHI] = S[0]; st[WS_GD] = S[1];
        wide_newton(S, kspan, a.nbin, pp, pd);
    } else {
        pp *= 0.5; pd *= 0.5;
    }
    st[WS_PPHI] = pp; st[WS_PD] = pd;
    st[WS_NEV] = (double)nev;
    if (fabs(pp) < kWideTol && fabs(pd) * kspan < kWideTol) {
        // (the last step is taken, not evaluated: the solution is the point it leads to)
        st[WS_PHI] += pp; st[WS_D] += pd;
        st[WS_STATUS] = 0.0;
        st[WS_DONE] = 1.0;
    } else if (nev >= kWideEvals) {
        st[WS_STATUS] = 1.0;
        st[WS_DONE] = 1.0;
    } else {
        st[WS_TPHI] = st[WS_PHI] + pp;
        st[WS_TD] = st[WS_D] + pd;
    }
}

__global__ __launch_bounds__(64) void k_wide_finish(WideArgs a) {
    __shared__ double S[kWidePart];
    const int s = blockIdx.x;
    const double *st = a.state + (int64_t)s * kWideState;
    const int nused = (int)st[WS_NUSED];
    wide_reduce(a, s, nused, S);
    if (threadIdx.x != 0) return;
    double *o = a.out + (int64_t)s * a.out_ld;
    // (phi_err^2, cov; cov, d_err^2) = (-H / 2)^-1
    const double a11 = -0.5 * S[2], a12 = -0.5 * S[3], a22 = -0.5 * S[4];
    const double det = a11 * a22 - a12 * a12;
    const bool degen = st[WS_STATUS] == 2.0 || !(a11 > 0.0 && det > 0.0);
    double phi = st[WS_PHI];
    phi -= rint(phi);
    if (phi >= 0.5) phi -= 1.0;
    const double inf = __builtin_huge_val();
    o[0] = phi;
    o[1] = degen ? inf : sqrt(a22 / det);
    o[2] = st[WS_D];
    o[3] = degen ? inf : sqrt(a11 / det);
    o[4] = degen ? 0.0 : -a12 / det;
    o[5] = S[8];
    o[6] = 2.0 * (double)a.K * (double)nused - (double)nused - 2.0;
    o[7] = (double)nused;
    o[8] = st[WS_NEV];
    o[9] = degen ? 2.0 : st[WS_STATUS];
}

// the stages of a fit, for pss_toa_wide_stages
enum { WIDE_SPECTRUM, WIDE_START, WIDE_ROUNDS, WIDE_FINISH };

template <int G>
static int launch_wide_rounds(const WideArgs &w, int first, int last, hipStream_t st) {
    const dim3 grid((unsigned)(w.nsub * w.nblk));
    if (first <= WIDE_ROUNDS && WIDE_ROUNDS <= last)
        for (int it = 0; it < kWideEvals; ++it) {
            k_wide_eval<G, false><<<grid, dim3(kWideT), 0, st>>>(w);
            k_wide_step<<<dim3((unsigned)w.nsub), dim3(64), 0, st>>>(w);
        }
    if (first <= WIDE_FINISH && WIDE_FINISH <= last) {
        k_wide_eval<G, true><<<grid, dim3(kWideT), 0, st>>>(w);
        k_wide_finish<<<dim3((unsigned)w.nsub), dim3(64), 0, st>>>(w);
    }
    LAUNCHCHK();
    return PSS_OK;
}

static bool wide_shape_ok(int32_t nchan, int32_t nsub, int32_t nbin, int32_t nharm, int32_t ndm) {
    return nchan >= 1 && nsub >= 1 && nbin >= 8 && nbin <= 8192 && nharm >= 1 && ndm >= 1 && ndm % 2 == 1;
}

extern "C" {

int64_t pss_toa_wide_workspace_bytes(int32_t nchan, int32_t nsub, int32_t nbin, int32_t nharm, int32_t ndm) {
    if (!wide_shape_ok(nchan, nsub, nbin, nharm, ndm)) return 0;
    return wide_layout(nchan, nsub, nbin, nharm, ndm).total;
}

int pss_toa_wide_stages(const float *data, int32_t nchan, int32_t nsub, int32_t nbin, int64_t ld, const float *tspec,
                        int32_t ntmpl, int32_t nharm, const double *kappa, const double *phi0, const float *wt,
                        int32_t ndm, double dm_step, double *out, int64_t out_ld, float *prof, int64_t prof_ld,
                        void *work, int64_t work_bytes, int32_t first, int32_t last, void *stream) {
    const char *what = first == WIDE_SPECTRUM && last == WIDE_FINISH ? "toa_wide_fit" : "toa_wide_stages";
    if (first < WIDE_SPECTRUM || last > WIDE_FINISH || first > last)
        return fail(PSS_EINVAL, "%s: stages %d .. %d are not within 0 .. 3", what, first, last);
    if (!data) return fail(PSS_EINVAL, "%s: data is NULL", what);
    if (!tspec) return fail(PSS_EINVAL, "%s: tspec is NULL", what);
    if (!kappa) return fail(PSS_EINVAL, "%s: kappa is NULL", what);
    if (!phi0) return fail(PSS_EINVAL, "%s: phi0 is NULL", what);
    if (!wt) return fail(PSS_EINVAL, "%s: wt is NULL", what);
    if (!out) return fail(PSS_EINVAL, "%s: out is NULL", what);
    if (!prof) return fail(PSS_EINVAL, "%s: prof is NULL", what);
    if (!work) return fail(PSS_EINVAL, "%s: work is NULL", what);
    if (nchan < 1) return fail(PSS_EINVAL, "%s: nchan %d < 1", what, nchan);
    if (nsub < 1) return fail(PSS_EINVAL, "%s: nsub %d < 1", what, nsub);
    if (nbin < 8 || nbin > 8192) return fail(PSS_EINVAL, "%s: nbin %d outside [8, 8192]", what, nbin);
    if (ld < (int64_t)nsub * nbin)
        return fail(PSS_EINVAL, "%s: ld %lld < nsub %d x nbin %d", what, (long long)ld, nsub, nbin);
    if (out_ld < 10) return fail(PSS_EINVAL, "%s: out_ld %lld < 10", what, (long long)out_ld);
    if (prof_ld < 4) return fail(PSS_EINVAL, "%s: prof_ld %lld < 4", what, (long long)prof_ld);
    if (ntmpl != 1 && ntmpl != nchan)
        return fail(PSS_EINVAL, "%s: ntmpl %d is neither 1 nor nchan %d", what, ntmpl, nchan);
    if (nharm < 1) return fail(PSS_EINVAL, "%s: nharm %d < 1", what, nharm);
    if (ndm < 1 || ndm % 2 == 0) return fail(PSS_EINVAL, "%s: ndm %d is not odd and >= 1", what, ndm);
    if (!(dm_step >= 0.0) || !(dm_step <= 1.7976931348623157e308))
        return fail(PSS_EINVAL, "%s: dm_step %g is not finite and >= 0", what, dm_step);
    const WideLayout L = wide_layout(nchan, nsub, nbin, nharm, ndm);
    if (work_bytes < L.total)
        return fail(PSS_EINVAL, "%s: a workspace of %lld bytes, %lld needed (pss_toa_wide_workspace_bytes)", what,
                    (long long)work_bytes, (long long)L.total);
    if ((uintptr_t)work % 16)
        return fail(PSS_EINVAL, "%s: the workspace is not on the 16-byte grid", what);
    const int nkb = (L.K - 1) / 64 + 1;
    if ((int64_t)nsub * L.nblk > 0x7fffffff || (int64_t)nsub * ndm * nkb > 0x7fffffff)
        return fail(PSS_EINVAL, "%s: %d sub-integrations x %d blocks or %d trials x %d exceed 2^31 - 1 workgroups", what,
                    nsub, L.nblk, ndm, nkb);
    hipStream_t st = (hipStream_t)stream;
    unsigned char *wb = static_cast<unsigned char *>(work);
    ToaArgs a;
    a.data = data; a.tspec = tspec; a.out = nullptr; a.ld = ld; a.out_ld = 0;
    a.nprof = (int64_t)nchan * nsub;
    a.nsub = nsub; a.nbin = nbin; a.K = L.K;
    a.per_chan = ntmpl != 1;
    a.wx = reinterpret_cast<cf *>(wb + L.x);
    a.wmeta = reinterpret_cast<double *>(wb + L.meta);
    a.nchan = nchan;
    if (first == WIDE_SPECTRUM) {
        const int rc = launch_toa<true>(what, a, on_grid16(data, ld) && nbin % 4 == 0, st);
        if (rc != PSS_OK) return rc;
    }
    WideArgs w;
    w.x = a.wx; w.meta = a.wmeta; w.kappa = kappa; w.phi0 = phi0; w.wt = wt;
    w.list = reinterpret_cast<int32_t *>(wb + L.list);
    w.xbar = reinterpret_cast<cf *>(wb + L.xbar);
    w.coarse = reinterpret_cast<float2 *>(wb + L.coarse);
    w.part = reinterpret_cast<double *>(wb + L.part);
    w.state = reinterpret_cast<double *>(wb + L.state);
    w.out = out; w.prof = prof; w.out_ld = out_ld; w.prof_ld = prof_ld;
    w.dm_step = dm_step;
    w.nchan = nchan; w.nsub = nsub; w.nbin = nbin; w.K = L.K; w.ndm = ndm; w.nblk = L.nblk; w.cb = L.cb;
    if (first <= WIDE_START && WIDE_START <= last) {
        k_wide_list<<<dim3((unsigned)nsub), dim3(64), 0, st>>>(w);
        const size_t bytes = (size_t)(nbin / 2 + 1) * 16 + (size_t)(L.K + 1) * 8;
        if (bytes > 65536)                                   // (dynamic LDS above 64 KB has to be asked for)
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_wide_coarse),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        k_wide_xbar<<<dim3((unsigned)(nsub * ndm * nkb)), dim3(64), 0, st>>>(w, nkb);
        k_wide_coarse<<<dim3((unsigned)(nsub * ndm)), dim3(kWideT), bytes, st>>>(w);
        k_wide_init<<<dim3(1), dim3(64), 0, st>>>(w);
        LAUNCHCHK();
    }
    switch (L.G) {
        case 64: return launch_wide_rounds<64>(w, first, last, st);
        case 16: return launch_wide_rounds<16>(w, first, last, st);
        default: return launch_wide_rounds<4>(w, first, last, st);
    }
}

int pss_toa_wide_fit(const float *data, int32_t nchan, int32_t nsub, int32_t nbin, int64_t ld, const float *tspec,
                     int32_t ntmpl, int32_t nharm, const double *kappa, const double *phi0, const float *wt,
                     int32_t ndm, double dm_step, double *out, int64_t out_ld, float *prof, int64_t prof_ld,
                     void *work, int64_t work_bytes, void *stream) {
    return pss_toa_wide_stages(data, nchan, nsub, nbin, ld, tspec, ntmpl, nharm, kappa, phi0, wt, ndm, dm_step, out,
                               out_ld, prof, prof_ld, work, work_bytes, WIDE_SPECTRUM, WIDE_FINISH, stream);
}

}  // extern "C"
