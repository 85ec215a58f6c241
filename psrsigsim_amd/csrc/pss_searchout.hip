// pss_searchout.hip -- search-mode PSRFITS output on the device (extension, no
// reference counterpart): per-block channel statistics and the quantised,
// time-major (channel fastest) sample stream a SUBINT row's DATA column holds.
//
//   k_chan_stats<VEC>       : min / max / sum / sum of squares of every
//                             (row, channel) block of nsblk samples; one wave
//                             per block, float64 sums in a fixed order.
//   k_quantize<NBITS, FAST> : data[c][t] float32 -> out[r][t][c] NBITS-bit
//                             codes; a 64-sample x 64-output-byte tile per
//                             workgroup pass, transposed through LDS as packed
//                             dwords.
#include "pss_common.hpp"

using namespace pss;

// ---------------------------------------------------------------------------
// statistics
// ---------------------------------------------------------------------------
// Sample i of a block belongs to lane (i / 4) % 64 and to that lane's
// accumulator i % 4, whatever the alignment (VEC only chooses 16-B loads), so
// the float64 sums are the same bits on the aligned and the ragged path:
// per accumulator in increasing i, then ((a0 + a1) + (a2 + a3)), then the xor
// butterfly 32, 16, .. 1 over the lanes.
struct Stat4 {
    double s[4], q[4];
    float lo, hi;
    bool nan;
};

__device__ __forceinline__ void stat_add(Stat4 &a, const float (&x)[4], int cnt) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < cnt) {
            const double d = (double)x[j];
            a.s[j] += d;
            a.q[j] += d * d;
            a.lo = fminf(a.lo, x[j]);
            a.hi = fmaxf(a.hi, x[j]);
            a.nan |= x[j] != x[j];
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void load4(const float *p, int64_t i, int64_t n, float (&x)[4]) {
    if (VEC) {
        const float4 v = *reinterpret_cast<const float4 *>(p + i);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = (i + j < n) ? p[i + j] : 0.0f;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_chan_stats(const float *__restrict__ data, int64_t ld, int32_t nchan,
                                                    int64_t nsblk, int64_t nrows, float *__restrict__ mn,
                                                    float *__restrict__ mx, double *__restrict__ sum,
                                                    double *__restrict__ sumsq) {
    const int c = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int64_t nq = (nsblk + 3) >> 2;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < nrows; r += (int64_t)gridDim.x * 4) {
        const float *p = data + (int64_t)c * ld + r * nsblk;
        Stat4 a;
#pragma unroll
        for (int j = 0; j < 4; ++j) a.s[j] = a.q[j] = 0.0;
        a.lo = INFINITY;
        a.hi = -INFINITY;
        a.nan = false;
        int64_t q = lane;
        for (; q + 192 < nq; q += 256) {       // four 16-B loads in flight per lane
            float x[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) load4<VEC>(p, (q + 64 * u) << 2, nsblk, x[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                stat_add(a, x[u], VEC ? 4 : (int)min((int64_t)4, nsblk - ((q + 64 * u) << 2)));
        }
        for (; q < nq; q += 64) {
            float x[4];
            load4<VEC>(p, q << 2, nsblk, x);
            stat_add(a, x, VEC ? 4 : (int)min((int64_t)4, nsblk - (q << 2)));
        }
        double s = (a.s[0] + a.s[1]) + (a.s[2] + a.s[3]);
        double s2 = (a.q[0] + a.q[1]) + (a.q[2] + a.q[3]);
        float lo = a.lo, hi = a.hi;
        int nan = a.nan ? 1 : 0;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            s += __shfl_xor(s, m);
            s2 += __shfl_xor(s2, m);
            lo = fminf(lo, __shfl_xor(lo, m));
            hi = fmaxf(hi, __shfl_xor(hi, m));
            nan |= __shfl_xor(nan, m);
        }
        if (lane == 0) {
            const int64_t o = r * nchan + c;
            mn[o] = nan ? NAN : lo;
            mx[o] = nan ? NAN : hi;
            sum[o] = nan ? (double)NAN : s;
            sumsq[o] = nan ? (double)NAN : s2;
        }
    }
}

// ---------------------------------------------------------------------------
// quantise + transpose
// ---------------------------------------------------------------------------
// A tile is QT = 64 time samples x QG = 16 output dwords (64 B of every time
// sample's channel run: 64 / 128 / 256 channels at 8 / 4 / 2 bits).  Thread
// (g, tq) of the load phase reads 4 consecutive samples of each of the CPD =
// 32 / NBITS channels of dword g (16 lanes cover 256 B of one channel),
// quantises them and packs one dword per sample; the four dwords go to LDS as
// one 16-B write at [g][4 tq].  The store phase reads dword [g][t] and writes
// it to out[t][4 g]: 16 lanes cover the tile's 64 B of one sample, a wave 4
// samples, so with nchan * NBITS / 8 a multiple of 64 every wave-level store
// is whole 64-B-aligned segments.  LDS rows are QT + 4 dwords: the 16-B writes
// stay aligned, and a 32-lane half of the store phase's reads (8 g x 4 t)
// falls on banks 4 g + t, all distinct.
enum { QT = 64, QG = 16, QLD = QT + 4 };

template <int NBITS>
__device__ __forceinline__ uint32_t quant1(float x, float offs, float inv) {
    const float r = rintf((x - offs) * inv);                   // round half to even
    // fmaxf / fminf return the non-NaN operand: a NaN x (or inf x 0) gives 0
    return (uint32_t)(int)fminf(fmaxf(r, 0.0f), (float)((1 << NBITS) - 1));
}

template <int NBITS, bool FAST>
__global__ __launch_bounds__(256) void k_quantize(const float *__restrict__ data, int64_t ld, int32_t nchan,
                                                  int64_t nsblk, int64_t nrows, const float *__restrict__ scl,
                                                  const float *__restrict__ offs, uint8_t *__restrict__ out) {
    constexpr int CPD = 32 / NBITS;                  // channels per output dword
    constexpr int PER = 8 / NBITS;                   // channels per output byte
    __shared__ __attribute__((aligned(16))) uint32_t tile[QG * QLD];
    const int64_t rowbytes = (int64_t)nchan * NBITS / 8;
    const int64_t byte0 = (int64_t)blockIdx.y * (QG * 4);       // tile's first byte of a sample's run
    const int64_t tiles_per_row = (nsblk + QT - 1) / QT;
    const int64_t ntiles = nrows * tiles_per_row;
    // load phase: dword g, samples 4 tq .. 4 tq + 3
    const int lg = threadIdx.x >> 4, ltq = threadIdx.x & 15;
    const int64_t lc0 = (byte0 + 4 * lg) * PER;                 // first channel of dword g
    // store phase: a 32-lane half holds 8 g x 4 t
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int sg = (lane & 7) + 8 * (lane >> 5), st = 4 * w + ((lane >> 3) & 3);
    for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int64_t r = tl / tiles_per_row;
        const int64_t t0 = (tl - r * tiles_per_row) * QT;
        const int64_t lt = t0 + 4 * ltq;
        uint32_t word[4] = {0u, 0u, 0u, 0u};
        if (lt < nsblk) {
            float x[CPD][4];
            float so[CPD], sinv[CPD];
#pragma unroll
            for (int k = 0; k < CPD; ++k) {
                const int64_t c = lc0 + k;
                if (c < nchan) {
                    load4<FAST>(data + c * ld + r * nsblk, lt, nsblk, x[k]);
                    const float s = scl[r * nchan + c];
                    so[k] = offs[r * nchan + c];
                    sinv[k] = s != 0.0f ? 1.0f / s : 0.0f;       // scl == 0: code 0
                } else {
                    x[k][0] = x[k][1] = x[k][2] = x[k][3] = 0.0f;
                    so[k] = sinv[k] = 0.0f;
                }
            }
#pragma unroll
            for (int k = 0; k < CPD; ++k) {
                // byte (k NBITS) / 8 of the dword; within it the lower-numbered
                // channel sits in the more significant bits
                const int sh = 8 * ((k * NBITS) / 8) + 8 - NBITS * ((k % PER) + 1);
#pragma unroll
                for (int j = 0; j < 4; ++j) word[j] |= quant1<NBITS>(x[k][j], so[k], sinv[k]) << sh;
            }
        }
        *reinterpret_cast<uint4 *>(&tile[lg * QLD + 4 * ltq]) = make_uint4(word[0], word[1], word[2], word[3]);
        __syncthreads();
        const int64_t sb = byte0 + 4 * sg;                        // this lane's byte of the sample's run
#pragma unroll
        for (int i = 0; i < QT / 16; ++i) {
            const int tt = 16 * i + st;
            const int64_t t = t0 + tt;
            if (t < nsblk && sb < rowbytes) {
                const uint32_t v = tile[sg * QLD + tt];
                uint8_t *o = out + (r * nsblk + t) * rowbytes + sb;
                if (FAST) {
                    *reinterpret_cast<uint32_t *>(o) = v;        // rowbytes % 4 == 0: whole dwords only
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (sb + b < rowbytes) o[b] = (uint8_t)(v >> (8 * b));
                }
            }
        }
        __syncthreads();
    }
}

template <int NBITS>
static int launch_quantize(const float *data, int64_t ld, int32_t nchan, int64_t nsblk, int64_t nrows,
                           const float *scl, const float *offs, uint8_t *out, hipStream_t st) {
    const int64_t rowbytes = (int64_t)nchan * NBITS / 8;
    const int64_t ntiles = nrows * ((nsblk + QT - 1) / QT);
    dim3 g = stream_grid(ntiles * 256, (int)((rowbytes + QG * 4 - 1) / (QG * 4)));
    // 16-B loads and whole-dword stores need the alignment; anything else
    // takes the element-wise path (same codes)
    const bool fast = on_grid16(data, ld) && nsblk % 4 == 0 && rowbytes % 4 == 0 && ((uintptr_t)out % 4 == 0);
    if (fast)
        k_quantize<NBITS, true><<<g, dim3(256), 0, st>>>(data, ld, nchan, nsblk, nrows, scl, offs, out);
    else
        k_quantize<NBITS, false><<<g, dim3(256), 0, st>>>(data, ld, nchan, nsblk, nrows, scl, offs, out);
    LAUNCHCHK();
    return PSS_OK;
}

extern "C" {

int pss_chan_stats(const float *data, int32_t nchan, int64_t ld, int64_t nsblk, int64_t nrows, float *mn,
                   float *mx, double *sum, double *sumsq, void *stream) {
    if (nsblk < 1) return fail(PSS_EINVAL, "chan_stats: nsblk %lld < 1", (long long)nsblk);
    if (nchan > 65535) return fail(PSS_EINVAL, "nchan %d > 65535 per launch", nchan);
    if (nchan <= 0 || nrows <= 0) return PSS_OK;
    if (!data || !mn || !mx || !sum || !sumsq) return fail(PSS_EINVAL, "chan_stats: NULL argument");
    if (nrows > ld / nsblk) return fail(PSS_EINVAL, "chan_stats: ld %lld < %lld rows of %lld samples", (long long)ld,
                                        (long long)nrows, (long long)nsblk);
    dim3 g = stream_grid((nrows + 3) / 4 * 256, nchan);
    const bool vec = on_grid16(data, ld) && nsblk % 4 == 0;
    if (vec)
        k_chan_stats<true><<<g, dim3(256), 0, (hipStream_t)stream>>>(data, ld, nchan, nsblk, nrows, mn, mx, sum, sumsq);
    else
        k_chan_stats<false><<<g, dim3(256), 0, (hipStream_t)stream>>>(data, ld, nchan, nsblk, nrows, mn, mx, sum, sumsq);
    LAUNCHCHK();
    return PSS_OK;
}

int pss_quantize_tmajor(const float *data, int32_t nchan, int64_t ld, int64_t nsblk, int64_t nrows,
                        const float *scl, const float *offs, int32_t nbits, void *out, void *stream) {
    if (nbits != 8 && nbits != 4 && nbits != 2) return fail(PSS_EINVAL, "quantize: nbits %d not 8, 4 or 2", nbits);
    if (nsblk < 1) return fail(PSS_EINVAL, "quantize: nsblk %lld < 1", (long long)nsblk);
    if (nchan > 65535) return fail(PSS_EINVAL, "nchan %d > 65535 per launch", nchan);
    if (nchan > 0 && ((int64_t)nchan * nbits) % 8)
        return fail(PSS_EINVAL, "quantize: %d channels of %d bits do not fill whole bytes", nchan, nbits);
    if (nchan <= 0 || nrows <= 0) return PSS_OK;
    if (!data || !scl || !offs || !out) return fail(PSS_EINVAL, "quantize: NULL argument");
    if (nrows > ld / nsblk) return fail(PSS_EINVAL, "quantize: ld %lld < %lld rows of %lld samples", (long long)ld,
                                        (long long)nrows, (long long)nsblk);
    hipStream_t st = (hipStream_t)stream;
    uint8_t *o = (uint8_t *)out;
    switch (nbits) {
        case 8: return launch_quantize<8>(data, ld, nchan, nsblk, nrows, scl, offs, o, st);
        case 4: return launch_quantize<4>(data, ld, nchan, nsblk, nrows, scl, offs, o, st);
        default: return launch_quantize<2>(data, ld, nchan, nsblk, nrows, scl, offs, o, st);
    }
}

}  // extern "C"
