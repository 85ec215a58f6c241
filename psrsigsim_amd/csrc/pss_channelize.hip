// pss_channelize.hip -- baseband channeliser / detector and amplitude noise
// (extensions, no reference counterpart for the channeliser; the noise is
// receiver.py:123-138's `norm * N(0, 1)`).
//
//   k_channelize<Chan<L, ...>, VL, VS> : voltages x[npol][n] -> detected powers
//       out[C][S], C = L / 2.  A workgroup owns GO consecutive output
//       time samples of every channel and walks their frames in order, BATCH
//       complex transforms of length L per pass on the Stockham engine of
//       pss_fft.hpp:
//         load   : y_m[j] = sum_t h[t L + j] x[(m + t) L + j] (the PFB taps
//                  applied while loading; T = 1 is the plain FFT filterbank),
//                  packed two real sequences per complex transform -- the two
//                  polarisations of one frame (npol = 2) or two consecutive
//                  frames (npol = 1) -- into LDS, natural order;
//         FFT    : registers + one LDS exchange per stage;
//         detect : one mirror read per bin.  npol = 2, Z = X_0 + i X_1:
//                  |X_0[k]|^2 + |X_1[k]|^2 = (|Z[k]|^2 + |Z[L-k]|^2) / 2;
//                  npol = 1: X_m[k] = (Z[k] + conj Z[L-k]) / 2 and
//                  X_{m+1}[k] = (Z[k] - conj Z[L-k]) / 2i.  The powers of the
//                  frames of one output sample are summed in frame order by
//                  ONE thread (no atomics: the same input gives the same bits)
//                  into the accumulators -- an LDS tile [C][GO] (C <= 512),
//                  or registers, C / threads channels x GO times (C >= 1024,
//                  where the tile does not fit beside the FFT buffer at a
//                  useful occupancy);
//         store  : the finished [C][GO] block goes to out[k][s0 ..] once:
//                  every channel row receives whole 64-B segments (GO is a
//                  multiple of 16 samples; the ragged tail stores elements).
//                  C = 4096 alone owns 4 samples per workgroup: more
//                  accumulators spill beside the 8192-point transform
//                  (DESIGN.md section 9 has the figures).
//       x is read from HBM once (plus the T - 1 halo frames of a workgroup;
//       the taps' re-reads of a pass hit the caches), out is written once,
//       and no spectra-major intermediate exists.
//   k_normal_add : rows[r][n] += scale * N(0, 1), the Philox Box-Muller normal
//       of the amplitude pulses (normal_x4), keyed (seed, call id, row, n).
#include <algorithm>

#include "pss_common.hpp"
#include "pss_fft.hpp"

using namespace pss;

struct ChanArgs {
    const float *x;
    int64_t n, ld;
    const float *h;
    int32_t npol, ntap, ts;
    float *out;
    int64_t out_ld, S, ngroups;
    float scale;       // 1 / (L tscrunch) times the packing's 1/2 (npol = 2) or 1/4 (npol = 1)
};

template <bool VEC>
__device__ __forceinline__ void ld4(const float *p, float (&v)[4]) {
    if (VEC) {
        const float4 q = *reinterpret_cast<const float4 *>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = p[i];
    }
}

// The two real sequences of a transform slot, 4 samples each (j % 4 == 0):
// ya[i] = sum_t h[t L + j + i] xa[t L + j + i], yb the same of xb (NULL: zeros);
// xa / xb point at sample 0 of the sequence's first frame.  One load of the
// taps serves both.
template <int L, bool VEC>
__device__ __forceinline__ void pfb4x2(const ChanArgs &a, const float *xa, const float *xb, int j, float (&ya)[4],
                                       float (&yb)[4]) {
    PSS_DASSERT(xa >= a.x && xa + (int64_t)a.ntap * L <= a.x + (a.npol - 1) * a.ld + a.n);
    const float *hp = a.h + j;
    for (int t = 0; t < a.ntap; ++t) {
        float hv[4], xv[4];
        ld4<VEC>(hp + t * L, hv);
        ld4<VEC>(xa + (int64_t)t * L + j, xv);
#pragma unroll
        for (int i = 0; i < 4; ++i) ya[i] = fmaf(hv[i], xv[i], ya[i]);
        if (xb) {
            ld4<VEC>(xb + (int64_t)t * L + j, xv);
#pragma unroll
            for (int i = 0; i < 4; ++i) yb[i] = fmaf(hv[i], xv[i], yb[i]);
        }
    }
}

// detected power of frame half `hh` of a slot from its bin pair (unscaled)
__device__ __forceinline__ float det_power(cf za, cf zb, bool two_pol, int hh) {
    if (two_pol) return fmaf(za.x, za.x, za.y * za.y) + fmaf(zb.x, zb.x, zb.y * zb.y);
    const float ux = hh ? za.x - zb.x : za.x + zb.x;
    const float uy = hh ? za.y + zb.y : za.y - zb.y;
    return fmaf(ux, ux, uy * uy);
}

// RG_: 0 = LDS tile accumulators; else the register accumulators' width (output
// samples per workgroup: 16 or 4)
template <int L_, int BATCH_, int T_, int RG_, typename F>
struct Chan;

template <int L_, int BATCH_, int T_, int RG_, int... F>
struct Chan<L_, BATCH_, T_, RG_, RList<F...>> {
    static constexpr int L = L_, BATCH = BATCH_, T = T_, C = L_ / 2;
    static constexpr bool REG = RG_ != 0;
    using FF = Fft<L, BATCH, T>;
    using LD = Lds<L>;
    static constexpr int E = FF::E;
    static constexpr int RF0 = FF::template first<F...>();
    static constexpr int RFL = FF::template last_of<F...>();
    // output samples per workgroup: a pass holds up to 2 BATCH frames (npol = 1)
    static constexpr int GO = REG ? RG_ : (2 * BATCH > 16 ? 2 * BATCH : 16);
    static constexpr int GA = REG ? RG_ : 1;      // accumulator registers per channel
    static constexpr int GP = GO + 1;            // tile pitch (odd: channel-fastest adds spread over the banks)
    static constexpr int NCH = REG ? C / T : 1;  // register mode: channels tid + i T
    static_assert(!REG || (BATCH == 1 && C % T == 0), "register accumulators: one transform per pass");

    // VL: 16-B loads of x and h; VS: 16-B stores of the register accumulators
    template <bool VL, bool VS>
    __device__ static void body(const ChanArgs &a) {
        __shared__ __align__(16) cf lds[BATCH * LD::RS];
        __shared__ float tile[REG ? 1 : C * GP];
        const int tid = threadIdx.x;
        const bool two = a.npol == 2;
        const int FP = two ? 1 : 2;                 // frames per transform slot
        for (int64_t g = blockIdx.x; g < a.ngroups; g += gridDim.x) {
            const int64_t s0 = g * GO;
            const int nout = (int)min((int64_t)GO, a.S - s0);
            const int64_t m0 = s0 * a.ts;           // first frame of the group
            const int64_t nfr = (int64_t)nout * a.ts;
            float acc[NCH][GA];
            if (REG) {
#pragma unroll
                for (int i = 0; i < NCH; ++i)
#pragma unroll
                    for (int s = 0; s < GA; ++s) acc[i][s] = 0.0f;
            } else {
                for (int it = tid; it < C * GP; it += T) tile[it] = 0.0f;
            }
            for (int64_t fa = 0; fa < nfr; fa += BATCH * FP) {
                const int nf = (int)min((int64_t)(BATCH * FP), nfr - fa);   // frames of this pass
                // ---- load: PFB-weighted frames -> LDS (natural order)
                for (int it = tid; it < BATCH * (L / 4); it += T) {
                    const int b = it / (L / 4);
                    const int j = (it - b * (L / 4)) * 4;
                    float re[4] = {0.0f, 0.0f, 0.0f, 0.0f}, im[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    const int f0 = b * FP;
                    if (f0 < nf) {
                        const float *xa = a.x + (m0 + fa + f0) * L;
                        const float *xb = two ? xa + a.ld : (f0 + 1 < nf ? xa + L : nullptr);
                        pfb4x2<L, VL>(a, xa, xb, j, re, im);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) lds[LD::at(b, j + i)] = make_float2(re[i], im[i]);
                }
                __syncthreads();
                {
                    cf v[E];
                    FF::template load<RF0>(v, lds, tid);
                    __syncthreads();
                    FF::template run<false, 1, F...>(v, lds, tid);
                    FF::template store<RFL>(v, lds, tid);
                }
                __syncthreads();
                // ---- detect
                if constexpr (REG) {
                    float p[NCH][2];
#pragma unroll
                    for (int i = 0; i < NCH; ++i) {
                        const int k = tid + i * T;
                        const cf za = lds[LD::at(0, k)];
                        const cf zb = lds[LD::at(0, (L - k) & (L - 1))];
                        p[i][0] = det_power(za, zb, two, 0);
                        p[i][1] = two ? 0.0f : det_power(za, zb, false, 1);
                    }
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) {
                        if (hh < nf) {
                            const int s = (int)((fa + hh) / a.ts);        // workgroup-uniform, < nout <= GA
#pragma unroll
                            for (int q = 0; q < GA; ++q) {
                                if (s == q) {
#pragma unroll
                                    for (int i = 0; i < NCH; ++i) acc[i][q] += p[i][hh];
                                }
                            }
                        }
                    }
                } else {
                    const int sa = (int)(fa / a.ts);
                    const int no = (int)((fa + nf - 1) / a.ts) - sa + 1;   // output samples this pass touches
                    for (int it = tid; it < C * no; it += T) {
                        const int gi = it / C, k = it - gi * C;
                        const int s = sa + gi;
                        const int64_t flo = max(fa, (int64_t)s * a.ts);
                        const int64_t fhi = min(fa + nf, ((int64_t)s + 1) * a.ts);
                        float sum = 0.0f;
                        for (int64_t f = flo; f < fhi; ++f) {
                            const int r = (int)(f - fa);
                            const int b = two ? r : (r >> 1), hh = two ? 0 : (r & 1);
                            const cf za = lds[LD::at(b, k)];
                            const cf zb = lds[LD::at(b, (L - k) & (L - 1))];
                            sum += det_power(za, zb, two, hh);
                        }
                        PSS_DASSERT(s < nout);
                        tile[k * GP + s] += sum;
                    }
                }
                __syncthreads();
            }
            // ---- store: out[k][s0 + s], s < nout
            if constexpr (REG) {
#pragma unroll
                for (int i = 0; i < NCH; ++i) {
                    float *o = a.out + (int64_t)(tid + i * T) * a.out_ld + s0;
                    if (VS && nout == GA) {
#pragma unroll
                        for (int q = 0; q < GA / 4; ++q)
                            *reinterpret_cast<float4 *>(o + 4 * q) =
                                make_float4(acc[i][4 * q] * a.scale, acc[i][4 * q + 1] * a.scale,
                                            acc[i][4 * q + 2] * a.scale, acc[i][4 * q + 3] * a.scale);
                    } else {
#pragma unroll
                        for (int s = 0; s < GA; ++s)
                            if (s < nout) o[s] = acc[i][s] * a.scale;
                    }
                }
            } else {
                for (int it = tid; it < C * GO; it += T) {
                    const int k = it / GO, s = it - k * GO;
                    if (s < nout) a.out[(int64_t)k * a.out_ld + s0 + s] = tile[k * GP + s] * a.scale;
                }
                __syncthreads();      // the next group zeroes the tile
            }
        }
    }
};

template <typename CH, bool VL, bool VS>
__global__ __launch_bounds__(CH::T) void k_channelize(ChanArgs a) { CH::template body<VL, VS>(a); }

template <typename CH, bool VL>
static void launch_channelize_vs(const ChanArgs &a, unsigned grid, bool vs, hipStream_t st) {
    if constexpr (CH::REG) {
        if (vs) {
            k_channelize<CH, VL, true><<<dim3(grid), dim3(CH::T), 0, st>>>(a);
            return;
        }
    }
    k_channelize<CH, VL, false><<<dim3(grid), dim3(CH::T), 0, st>>>(a);
}

template <typename CH>
static int launch_channelize(const ChanArgs &a0, hipStream_t st) {
    ChanArgs a = a0;
    a.ngroups = (a.S + CH::GO - 1) / CH::GO;
    const unsigned grid = (unsigned)std::min<int64_t>(a.ngroups, (int64_t)1 << 20);
    // decided separately: the 16-B loads need x, ld and h on the 16-B grid; the
    // 16-B stores (register accumulators only: the LDS-tile kernels store
    // dwords, 16 lanes along time) need out and out_ld there.  Same bits.
    const bool vl = on_grid16(a.x, a.ld) && ((uintptr_t)a.h % 16 == 0);
    const bool vs = on_grid16(a.out, a.out_ld);
    if (vl) launch_channelize_vs<CH, true>(a, grid, vs, st);
    else launch_channelize_vs<CH, false>(a, grid, vs, st);
    LAUNCHCHK();
    return PSS_OK;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_normal_add(float *__restrict__ rows, int64_t n, int64_t ld, float scale,
                                                    uint64_t seed, uint32_t call_id) {
    const uint32_t r = blockIdx.y;
    float *row = rows + (int64_t)r * ld;
    const Rng g(seed, call_id, P_NOISE);
    const int64_t items = (n + 3) >> 2;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items;
         it += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n0 = it << 2;
        // (Philox block n >> 2 holds samples 4 (n >> 2) .. + 3, as the amplitude pulses' draws)
        const float4 z = normal_x4(g.bits((uint32_t)(n0 >> 2), r, (uint32_t)(n0 >> 34)));
        if (VEC && n0 + 4 <= n) {                 // (row base and ld on the 16-B grid: host-selected)
            float4 d = *reinterpret_cast<const float4 *>(row + n0);
            d.x = fmaf(scale, z.x, d.x);
            d.y = fmaf(scale, z.y, d.y);
            d.z = fmaf(scale, z.z, d.z);
            d.w = fmaf(scale, z.w, d.w);
            *reinterpret_cast<float4 *>(row + n0) = d;
        } else {
            const float zz[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (n0 + i < n) row[n0 + i] = fmaf(scale, zz[i], row[n0 + i]);
        }
    }
}

extern "C" {

int pss_channelize(const float *x, int32_t npol, int64_t n, int64_t ld, const float *h, int32_t nchan, int32_t ntap,
                   int32_t tscrunch, float *out, int64_t out_ld, void *stream) {
    if (!x || !h || !out) return fail(PSS_EINVAL, "channelize: NULL argument");
    if (npol != 1 && npol != 2) return fail(PSS_EINVAL, "channelize: npol %d not 1 or 2", npol);
    if (nchan < 16 || nchan > 4096 || !is_pow2(nchan))
        return fail(PSS_EINVAL, "channelize: nchan %d not a power of two in [16, 4096]", nchan);
    if (ntap < 1 || ntap > 8) return fail(PSS_EINVAL, "channelize: ntap %d outside [1, 8]", ntap);
    if (tscrunch < 1) return fail(PSS_EINVAL, "channelize: tscrunch %d < 1", tscrunch);
    if (n < 0 || ld < n) return fail(PSS_EINVAL, "channelize: ld %lld < n %lld", (long long)ld, (long long)n);
    const int64_t L = 2 * (int64_t)nchan;
    const int64_t M = n / L - ntap + 1;
    const int64_t S = M > 0 ? M / tscrunch : 0;
    if (out_ld < S) return fail(PSS_EINVAL, "channelize: out_ld %lld < %lld output samples", (long long)out_ld,
                                (long long)S);
    if (S < 1) return PSS_OK;
    ChanArgs a;
    a.x = x; a.n = n; a.ld = ld; a.h = h; a.npol = npol; a.ntap = ntap; a.ts = tscrunch;
    a.out = out; a.out_ld = out_ld; a.S = S; a.ngroups = 0;
    a.scale = (float)((npol == 2 ? 0.5 : 0.25) / ((double)L * (double)tscrunch));
    hipStream_t st = (hipStream_t)stream;
    switch (nchan) {
        case 16: return launch_channelize<Chan<32, 128, 256, 0, C32F>>(a, st);
        case 32: return launch_channelize<Chan<64, 64, 256, 0, C64F>>(a, st);
        case 64: return launch_channelize<Chan<128, 32, 256, 0, C128F>>(a, st);
        case 128: return launch_channelize<Chan<256, 16, 256, 0, C256>>(a, st);
        case 256: return launch_channelize<Chan<512, 8, 256, 0, C512F>>(a, st);
        case 512: return launch_channelize<Chan<1024, 4, 256, 0, C1kF>>(a, st);
        case 1024: return launch_channelize<Chan<2048, 1, 256, 16, RList<8, 8, 8, 4>>>(a, st);
        case 2048: return launch_channelize<Chan<4096, 1, 512, 16, RList<8, 8, 8, 8>>>(a, st);
        // (4 samples per workgroup: beside the transform's registers 8 channels x 8 accumulators already spill
        // at the 256 registers a 512-thread workgroup has)
        default: return launch_channelize<Chan<8192, 1, 512, 4, C8kF>>(a, st);
    }
}

int pss_normal_add(float *rows, int32_t nrows, int64_t n, int64_t ld, float scale, uint64_t seed, uint32_t call_id,
                   void *stream) {
    if (nrows > 65535) return fail(PSS_EINVAL, "normal_add: %d rows > 65535 per launch", nrows);
    if (n < 0 || ld < n) return fail(PSS_EINVAL, "normal_add: ld %lld < n %lld", (long long)ld, (long long)n);
    if (nrows <= 0 || n == 0) return PSS_OK;
    if (!rows) return fail(PSS_EINVAL, "normal_add: NULL argument");
    const dim3 g = stream_grid((n + 3) / 4, nrows);
    if (on_grid16(rows, ld))
        k_normal_add<true><<<g, dim3(256), 0, (hipStream_t)stream>>>(rows, n, ld, scale, seed, call_id);
    else
        k_normal_add<false><<<g, dim3(256), 0, (hipStream_t)stream>>>(rows, n, ld, scale, seed, call_id);
    LAUNCHCHK();
    return PSS_OK;
}

}  // extern "C"
