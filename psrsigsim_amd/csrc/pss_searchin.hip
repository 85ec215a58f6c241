// pss_searchin.hip -- search-mode PSRFITS input on the device (extension, no
// reference counterpart): the inverse of pss_searchout.hip's quantiser.
//
//   k_unpack<NBITS, NSUM, FAST> : in[r][t][p][c] NBITS-bit codes (channel
//                                 fastest, as a SUBINT row's DATA column holds
//                                 them) -> out[c][r nsblk + t] float32; a
//                                 64-sample x 64-input-byte tile per workgroup
//                                 pass, transposed through LDS as packed dwords
//                                 (DESIGN.md section 9).
#include "pss_common.hpp"

using namespace pss;

// A tile is UT = 64 time samples x UG = 16 input dwords (64 B of one
// polarisation's channel run of every sample: 64 / 128 / 256 channels at 8 / 4
// / 2 bits), the quantiser's tile read the other way.  Load phase: thread
// (t, g) reads dword in[..][t][p][4 g] -- 16 lanes cover the tile's 64 B of one
// sample, a wave 4 samples -- and writes it to LDS at [p][g][t]; 4 steps cover
// the 64 samples.  Store phase: thread (g, tq) reads dwords [g][4 tq .. 4 tq +
// 3] of each summed polarisation as one 16-B LDS read, decodes the CPD = 32 /
// NBITS channels of dword g and writes one float4 per channel at out[c][r
// nsblk + t0 + 4 tq]: 16 lanes write 256 contiguous bytes of a channel row.
// The narrow 64-B segments are reads here and every write is a whole run (the
// quantiser has it the other way round).  LDS rows are UT + 4 dwords: the
// 16-B reads stay aligned, and a 32-lane half of the load phase's writes (16 g
// x 2 t) falls on banks 4 g + t mod 32, two lanes each, which a 4-B LDS write
// absorbs.  The memory fetches 128-B lines, of which a tile uses half: a
// workgroup therefore takes UW = 2 tiles side by side one after the other, and
// the second finds its lines in the cache.
enum { UT = 64, UG = 16, ULD = UT + 4, UW = 2 };

// value of one code (include/pss_hip.h): explicit fmaf, nothing for
// -ffp-contract to decide
__device__ __forceinline__ float dequant(uint32_t code, float zero_off, float s, float o) {
    return fmaf((float)code - zero_off, s, o);
}

template <int NBITS, int NSUM, bool FAST>
__global__ __launch_bounds__(256) void k_unpack(const uint8_t *__restrict__ in, int32_t nchan, int32_t npol,
                                                int64_t nsblk, int64_t nrows, const float *__restrict__ scl,
                                                const float *__restrict__ offs, const float *__restrict__ wts,
                                                float zero_off, int32_t flip, float *__restrict__ out, int64_t ld) {
    constexpr int CPD = 32 / NBITS;                  // channels per input dword
    constexpr int PER = 8 / NBITS;                   // channels per input byte
    constexpr uint32_t MASK = (1u << NBITS) - 1u;
    __shared__ __attribute__((aligned(16))) uint32_t tile[NSUM][UG * ULD];
    const int64_t rowbytes = (int64_t)nchan * NBITS / 8;        // one polarisation of one sample
    const int64_t sampbytes = rowbytes * npol;
    const int64_t tiles_per_row = (nsblk + UT - 1) / UT;
    const int64_t ntiles = nrows * tiles_per_row;
    // load phase: dword g of samples lt, lt + 16, lt + 32, lt + 48
    const int lg = threadIdx.x & 15, lt = threadIdx.x >> 4;
    // store phase: dword g, samples 4 tq .. 4 tq + 3
    const int sg = threadIdx.x >> 4, stq = threadIdx.x & 15;
    for (int64_t tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int64_t r = tl / tiles_per_row;
        const int64_t t0 = (tl - r * tiles_per_row) * UT;
        // the UW tiles side by side, one after the other: the second finds the
        // 128-B lines the first fetched in the cache
        for (int h = 0; h < UW; ++h) {
            // tile's first byte of a polarisation's run
            const int64_t byte0 = ((int64_t)blockIdx.y * UW + h) * (UG * 4);
            if (byte0 >= rowbytes) break;                       // (the whole workgroup leaves together)
            const int64_t lb = byte0 + 4 * lg;                  // this lane's byte of the run
            const int64_t sc0 = (byte0 + 4 * sg) * PER;         // first channel of dword g
#pragma unroll
            for (int p = 0; p < NSUM; ++p) {
                uint32_t v[UT / 16];
#pragma unroll
                for (int i = 0; i < UT / 16; ++i) {
                    const int64_t t = t0 + 16 * i + lt;
                    v[i] = 0u;
                    if (t < nsblk && lb < rowbytes) {
                        const uint8_t *q = in + (r * nsblk + t) * sampbytes + p * rowbytes + lb;
                        if (FAST) {
                            v[i] = *reinterpret_cast<const uint32_t *>(q);   // rowbytes % 4 == 0: whole dwords only
                        } else {
#pragma unroll
                            for (int b = 0; b < 4; ++b)
                                if (lb + b < rowbytes) v[i] |= (uint32_t)q[b] << (8 * b);
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < UT / 16; ++i) tile[p][lg * ULD + 16 * i + lt] = v[i];
            }
            __syncthreads();
            const int64_t t = t0 + 4 * stq;
            if (t < nsblk) {
                uint4 word[NSUM];
#pragma unroll
                for (int p = 0; p < NSUM; ++p) word[p] = *reinterpret_cast<const uint4 *>(&tile[p][sg * ULD + 4 * stq]);
#pragma unroll
                for (int k = 0; k < CPD; ++k) {
                    const int64_t c = sc0 + k;
                    if (c < nchan) {
                        // byte (k NBITS) / 8 of the dword; within it the lower-numbered
                        // channel sits in the more significant bits
                        const int sh = 8 * ((k * NBITS) / 8) + 8 - NBITS * ((k % PER) + 1);
                        float x[4];
#pragma unroll
                        for (int p = 0; p < NSUM; ++p) {
                            const int64_t so = (r * npol + p) * nchan + c;
                            const float s = scl[so], o = offs[so];
                            const uint32_t wd[4] = {word[p].x, word[p].y, word[p].z, word[p].w};
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                const float vp = dequant((wd[j] >> sh) & MASK, zero_off, s, o);
                                x[j] = p == 0 ? vp : x[j] + vp;
                            }
                        }
                        const float w = wts ? wts[r * nchan + c] : 1.0f;
#pragma unroll
                        for (int j = 0; j < 4; ++j) x[j] *= w;
                        float *o = out + (flip ? nchan - 1 - c : c) * ld + r * nsblk + t;
                        if (FAST) {
                            *reinterpret_cast<float4 *>(o) = make_float4(x[0], x[1], x[2], x[3]);
                        } else {
#pragma unroll
                            for (int j = 0; j < 4; ++j)
                                if (t + j < nsblk) o[j] = x[j];
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
}

struct UnpackArgs {
    const uint8_t *in;
    int32_t nchan, npol;
    int64_t nsblk, nrows;
    const float *scl, *offs, *wts;
    float zero_off;
    int32_t flip;
    float *out;
    int64_t ld;
};

template <int NBITS, int NSUM>
static int launch_unpack(const UnpackArgs &a, hipStream_t st) {
    const int64_t rowbytes = (int64_t)a.nchan * NBITS / 8;
    const int64_t ntiles = a.nrows * ((a.nsblk + UT - 1) / UT);
    dim3 g = stream_grid(ntiles * 256, (int)((rowbytes + UW * UG * 4 - 1) / (UW * UG * 4)));
    // whole-dword loads and 16-B stores need the alignment; anything else
    // takes the element-wise path (same bits)
    const bool fast = on_grid16(a.out, a.ld) && a.nsblk % 4 == 0 && rowbytes % 4 == 0 && ((uintptr_t)a.in % 4 == 0);
    if (fast)
        k_unpack<NBITS, NSUM, true><<<g, dim3(256), 0, st>>>(a.in, a.nchan, a.npol, a.nsblk, a.nrows, a.scl, a.offs,
                                                             a.wts, a.zero_off, a.flip, a.out, a.ld);
    else
        k_unpack<NBITS, NSUM, false><<<g, dim3(256), 0, st>>>(a.in, a.nchan, a.npol, a.nsblk, a.nrows, a.scl, a.offs,
                                                              a.wts, a.zero_off, a.flip, a.out, a.ld);
    LAUNCHCHK();
    return PSS_OK;
}

template <int NBITS>
static int launch_unpack_nsum(const UnpackArgs &a, int32_t nsum, hipStream_t st) {
    return nsum == 2 ? launch_unpack<NBITS, 2>(a, st) : launch_unpack<NBITS, 1>(a, st);
}

extern "C" {

int pss_unpack_tmajor(const void *in, int32_t nchan, int32_t npol, int32_t nsum, int64_t nsblk, int64_t nrows,
                      const float *scl, const float *offs, const float *wts, float zero_off, int32_t nbits,
                      int32_t flip, float *out, int64_t ld, void *stream) {
    if (nbits != 8 && nbits != 4 && nbits != 2) return fail(PSS_EINVAL, "unpack: nbits %d not 8, 4 or 2", nbits);
    if (npol != 1 && npol != 2 && npol != 4) return fail(PSS_EINVAL, "unpack: npol %d not 1, 2 or 4", npol);
    if (nsum < 1 || nsum > 2 || nsum > npol)
        return fail(PSS_EINVAL, "unpack: nsum %d not 1 or 2, or above npol %d", nsum, npol);
    if (nsblk < 1) return fail(PSS_EINVAL, "unpack: nsblk %lld < 1", (long long)nsblk);
    if (nchan > 65535) return fail(PSS_EINVAL, "nchan %d > 65535 per launch", nchan);
    if (nchan > 0 && ((int64_t)nchan * nbits) % 8)
        return fail(PSS_EINVAL, "unpack: %d channels of %d bits do not fill whole bytes", nchan, nbits);
    if (nchan <= 0 || nrows <= 0) return PSS_OK;
    if (!in || !scl || !offs || !out) return fail(PSS_EINVAL, "unpack: NULL argument");
    if (nrows > ld / nsblk) return fail(PSS_EINVAL, "unpack: ld %lld < %lld rows of %lld samples", (long long)ld,
                                        (long long)nrows, (long long)nsblk);
    const UnpackArgs a = {(const uint8_t *)in, nchan, npol, nsblk, nrows, scl, offs, wts, zero_off, flip != 0, out, ld};
    hipStream_t st = (hipStream_t)stream;
    switch (nbits) {
        case 8: return launch_unpack_nsum<8>(a, nsum, st);
        case 4: return launch_unpack_nsum<4>(a, nsum, st);
        default: return launch_unpack_nsum<2>(a, nsum, st);
    }
}

}  // extern "C"
