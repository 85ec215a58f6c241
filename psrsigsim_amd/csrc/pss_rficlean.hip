// pss_rficlean.hip -- RFI excision of a [chan][time] search-mode filterbank
// (extension, no reference counterpart): replace the flagged (block, channel)
// cells of a mask by the channel's baseline and, with zero_dm, remove the
// band-averaged (zero-DM) time series of the unflagged channels.
//
//   b(t)      = min(t / block, nblk - 1)        (the ragged tail joins the last block)
//   good(c,t) = !mask[b(t) * nchan + c]
//   zero_dm = 0:  out[c][t] = good ? data[c][t] : base[c]
//   zero_dm = 1:  S[t]      = sum_{c good} (data[c][t] - base[c])
//                 z[t]      = S[t] * rgood[b(t)]
//                 out[c][t] = good ? data[c][t] - z[t] : base[c]
//                 zser[t]   = z[t]
//
// every line one rounded IEEE float32 operation; the kernel never divides.
//
//   k_rfi_clean<VIN, VOUT, ZDM> : a workgroup of 512 threads (kRfQ = 8 waves)
//       owns kRfTile = 256 consecutive times of every channel.  Lanes run
//       along time, 4 consecutive samples per lane; wave q owns the contiguous
//       channel range
//           [q P, min((q + 1) P, nchan)),   P = ceil(nchan / 8)
//       (empty for the last waves when nchan is small).
//
//       SUMMATION ORDER (a pure function of nchan; part of the contract): each
//       of the 8 ranges is summed in increasing c into one accumulator that
//       starts at +0,  A_q = (..((0 + d_c0) + d_c1) ..),  d_c = data[c][t] -
//       base[c], a flagged cell is skipped (it is never added, so a NaN or
//       1e30 in it reaches nothing), and the eight partial sums are combined
//       through LDS as
//           S = ((A_0 + A_1) + (A_2 + A_3)) + ((A_4 + A_5) + (A_6 + A_7)).
//       It depends on neither n, block, the alignment, the tile, zser nor the
//       run.  No atomics, no workspace.
//
//       zero_dm makes two passes over the tile: the sum, a barrier, then every
//       wave reads its rows again (from the XCD's L2 when the tile's
//       nchan KiB of the workgroups resident there fit into it), subtracts and
//       stores.  zero_dm = 0 is the second pass alone; in place it writes the
//       flagged cells only.  Nothing of `out` is written before the whole
//       tile has been summed and tiles are disjoint in time, so out == data
//       gives the bits of the out-of-place run.
//
//       The mask byte of a channel is wave-uniform when the tile lies in one
//       block (always, for block a multiple of 256): the wave then loads the
//       bytes of 64 channels at once, one per lane, and a ballot makes them a
//       scalar bit set -- uniform branches, a flagged row is not even loaded.
//       16 rows (the sum) or 8 (the storing pass) are in flight per wave.  A
//       tile that straddles a border looks its four bytes up per lane (a
//       lane's 4 samples may lie in two blocks when block % 4 != 0).  VIN / VOUT choose 16-B loads / stores for rows on the 16-B
//       grid, dwords otherwise and for the ragged last quad -- the same
//       values.  Workgroup id -> time tile through the XCD run map.
#include "pss_common.hpp"

using namespace pss;

static constexpr int kRfQ = 8;                        // waves = channel ranges per workgroup
static constexpr int kRfThreads = 64 * kRfQ;
static constexpr int kRfS = 4;                        // consecutive samples per lane
static constexpr int kRfTile = 64 * kRfS;             // times per workgroup
static constexpr int kRfU1 = 16;                      // channels in flight per wave: the sum,
static constexpr int kRfU = 8;                        //   and the pass that stores
static_assert(64 % kRfU1 == 0 && 64 % kRfU == 0, "a batch stays inside one 64-channel flag set");

struct RfArgs {
    int64_t n, ld, out_ld, block, nblk;
    int32_t nchan, per, inplace;
};

// x[k] = row[t + k] (k < 4), zeros at and past n: one 16-B load for a whole
// quad of a row on the grid, dwords otherwise
template <bool VEC>
__device__ __forceinline__ void rf_load4(const float *row, int64_t t, int64_t n, bool full, float (&x)[kRfS]) {
    if (VEC && full) {
        const float4 v = *reinterpret_cast<const float4 *>(row + t);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < kRfS; ++k) x[k] = (t + k < n) ? row[t + k] : 0.0f;
    }
}

template <bool VEC>
__device__ __forceinline__ void rf_store4(float *row, int64_t t, int64_t n, bool full, const float (&y)[kRfS]) {
    if (VEC && full) {
        *reinterpret_cast<float4 *>(row + t) = make_float4(y[0], y[1], y[2], y[3]);
    } else {
#pragma unroll
        for (int k = 0; k < kRfS; ++k)
            if (t + k < n) row[t + k] = y[k];
    }
}

// The mask bytes of the 64 channels [cb, cb + 64) of one block as a wave-uniform
// bit set (bit i: channel cb + i is flagged, or at / past c_hi): one byte load
// per lane and a ballot, instead of a dependent load in front of every row
__device__ __forceinline__ uint64_t rf_flags(const uint8_t *mrow, int cb, int c_hi, int lane) {
    const int c = cb + lane;
    return __ballot(c < c_hi ? mrow[c] != 0 : true);
}

// (data and out may be the same rows: neither is __restrict__)
template <bool VIN, bool VOUT, bool ZDM>
__global__ __launch_bounds__(kRfThreads) void k_rfi_clean(const float *data, const uint8_t *__restrict__ mask,
                                                          const float *__restrict__ base,
                                                          const float *__restrict__ rgood, float *out, float *zser,
                                                          RfArgs a) {
    __shared__ __align__(16) float part[kRfQ][kRfTile];
    const int tid = threadIdx.x, q = tid >> 6, lane = tid & 63;
    const int64_t t0 = (int64_t)xcd_run_id() * kRfTile;        // < n: the grid is ceil(n / kRfTile)
    const int64_t t = t0 + lane * kRfS;
    const bool full = t + kRfS <= a.n;
    const int c_lo = min(q * a.per, a.nchan), c_hi = min(c_lo + a.per, a.nchan);
    // the tile's first and last block (wave-uniform)
    const int64_t bq = t0 / a.block;
    const int64_t r0 = t0 - bq * a.block;
    const int64_t bf = min(bq, a.nblk - 1);
    const int64_t bl = min((min(t0 + kRfTile, a.n) - 1) / a.block, a.nblk - 1);
    const bool one_block = bf == bl;
    // the block of each of the lane's samples (valid for a sample past n too)
    int64_t mo[kRfS];
    float rg[kRfS];
#pragma unroll
    for (int k = 0; k < kRfS; ++k) {
        int64_t b = bf;
        if (!one_block) {
            // r0 < block and the offset < 256: the quotient is 1 for a block beyond 32 bits
            const int64_t v = r0 + lane * kRfS + k;
            const int64_t up = v < a.block ? 0 : ((a.block >> 31) ? 1 : (int64_t)((uint32_t)v / (uint32_t)a.block));
            b = min(bq + up, a.nblk - 1);
        }
        mo[k] = b * a.nchan;
        rg[k] = ZDM ? rgood[b] : 0.0f;
    }
    const uint8_t *mrow = mask + bf * a.nchan;                 // the one block's row of the mask

    float z[kRfS] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ZDM) {
        float acc[kRfS] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (one_block) {
            for (int cb = c_lo; cb < c_hi; cb += 64) {
                const uint64_t flg = rf_flags(mrow, cb, c_hi, lane);
                for (int c = cb; c < min(cb + 64, c_hi); c += kRfU1) {
                    float x[kRfU1][kRfS], bs[kRfU1];
                    bool g[kRfU1];
#pragma unroll
                    for (int u = 0; u < kRfU1; ++u) {
                        const int cc = c + u;
                        g[u] = !((flg >> (cc - cb)) & 1);
                        if (g[u]) {
                            rf_load4<VIN>(data + (int64_t)cc * a.ld, t, a.n, full, x[u]);
                            bs[u] = base[cc];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < kRfU1; ++u) {
                        if (g[u]) {
#pragma unroll
                            for (int k = 0; k < kRfS; ++k) {
                                const float d = x[u][k] - bs[u];
                                acc[k] = acc[k] + d;
                            }
                        }
                    }
                }
            }
        } else {
            for (int c = c_lo; c < c_hi; ++c) {
                float x[kRfS];
                rf_load4<VIN>(data + (int64_t)c * a.ld, t, a.n, full, x);
                const float bs = base[c];
#pragma unroll
                for (int k = 0; k < kRfS; ++k) {
                    const float d = x[k] - bs;
                    const float s = acc[k] + d;
                    acc[k] = mask[mo[k] + c] ? acc[k] : s;     // (a select: a flagged NaN is dropped)
                }
            }
        }
        *reinterpret_cast<float4 *>(&part[q][lane * kRfS]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        __syncthreads();
        float p[kRfQ][kRfS];
#pragma unroll
        for (int i = 0; i < kRfQ; ++i) {
            const float4 v = *reinterpret_cast<const float4 *>(&part[i][lane * kRfS]);
            p[i][0] = v.x; p[i][1] = v.y; p[i][2] = v.z; p[i][3] = v.w;
        }
#pragma unroll
        for (int k = 0; k < kRfS; ++k) {
            const float s01 = p[0][k] + p[1][k], s23 = p[2][k] + p[3][k];
            const float s45 = p[4][k] + p[5][k], s67 = p[6][k] + p[7][k];
            const float lo = s01 + s23, hi = s45 + s67;
            const float s = lo + hi;
            z[k] = s * rg[k];
        }
        if (zser && q == 0) {
#pragma unroll
            for (int k = 0; k < kRfS; ++k)
                if (t + k < a.n) zser[t + k] = z[k];
        }
    }

    const bool flagged_only = !ZDM && a.inplace;               // a good cell keeps its value
    if (one_block) {
        for (int cb = c_lo; cb < c_hi; cb += 64) {
            const uint64_t flg = rf_flags(mrow, cb, c_hi, lane);
            for (int c = cb; c < min(cb + 64, c_hi); c += kRfU) {
                float x[kRfU][kRfS];
                int f[kRfU];                                   // 1 flagged, 0 good, -1 past the range
#pragma unroll
                for (int u = 0; u < kRfU; ++u) {
                    const int cc = c + u;
                    f[u] = cc < c_hi ? (int)((flg >> (cc - cb)) & 1) : -1;
                    if (f[u] == 0 && !flagged_only) rf_load4<VIN>(data + (int64_t)cc * a.ld, t, a.n, full, x[u]);
                }
#pragma unroll
                for (int u = 0; u < kRfU; ++u) {
                    const int cc = c + u;
                    if (f[u] < 0 || (f[u] == 0 && flagged_only)) continue;
                    float y[kRfS];
                    if (f[u]) {
                        const float bs = base[cc];
#pragma unroll
                        for (int k = 0; k < kRfS; ++k) y[k] = bs;
                    } else {
#pragma unroll
                        for (int k = 0; k < kRfS; ++k) y[k] = ZDM ? x[u][k] - z[k] : x[u][k];
                    }
                    rf_store4<VOUT>(out + (int64_t)cc * a.out_ld, t, a.n, full, y);
                }
            }
        }
    } else {
        for (int c = c_lo; c < c_hi; ++c) {
            float x[kRfS], y[kRfS];
            rf_load4<VIN>(data + (int64_t)c * a.ld, t, a.n, full, x);
            const float bs = base[c];
#pragma unroll
            for (int k = 0; k < kRfS; ++k) {
                const float v = ZDM ? x[k] - z[k] : x[k];
                y[k] = mask[mo[k] + c] ? bs : v;
            }
            rf_store4<VOUT>(out + (int64_t)c * a.out_ld, t, a.n, full, y);
        }
    }
}

template <bool VIN, bool VOUT>
static void rf_launch(dim3 grid, hipStream_t st, bool zdm, const float *data, const uint8_t *mask, const float *base,
                      const float *rgood, float *out, float *zser, const RfArgs &a) {
    if (zdm)
        k_rfi_clean<VIN, VOUT, true><<<grid, dim3(kRfThreads), 0, st>>>(data, mask, base, rgood, out, zser, a);
    else
        k_rfi_clean<VIN, VOUT, false><<<grid, dim3(kRfThreads), 0, st>>>(data, mask, base, rgood, out, zser, a);
}

extern "C" {

int pss_rfi_clean(const float *data, int32_t nchan, int64_t n, int64_t ld, const uint8_t *mask, int64_t block,
                  int64_t nblk, const float *base, const float *rgood, int32_t zero_dm, float *out, int64_t out_ld,
                  float *zser, void *stream) {
    if (!data) return fail(PSS_EINVAL, "rfi_clean: data is NULL");
    if (!mask) return fail(PSS_EINVAL, "rfi_clean: mask is NULL");
    if (!base) return fail(PSS_EINVAL, "rfi_clean: base is NULL");
    if (!out) return fail(PSS_EINVAL, "rfi_clean: out is NULL");
    if (zero_dm != 0 && zero_dm != 1) return fail(PSS_EINVAL, "rfi_clean: zero_dm %d is not 0 or 1", zero_dm);
    if (zero_dm && !rgood) return fail(PSS_EINVAL, "rfi_clean: rgood is NULL with zero_dm = 1");
    if (nchan < 1) return fail(PSS_EINVAL, "rfi_clean: nchan %d < 1", nchan);
    if (n < 1) return fail(PSS_EINVAL, "rfi_clean: n %lld < 1", (long long)n);
    if (ld < n) return fail(PSS_EINVAL, "rfi_clean: ld %lld < n %lld", (long long)ld, (long long)n);
    if (out_ld < n) return fail(PSS_EINVAL, "rfi_clean: out_ld %lld < n %lld", (long long)out_ld, (long long)n);
    if (block < 1) return fail(PSS_EINVAL, "rfi_clean: block %lld < 1", (long long)block);
    if (nblk < 1) return fail(PSS_EINVAL, "rfi_clean: nblk %lld < 1", (long long)nblk);
    // (nblk - 1) * block >= n, without the product
    if (nblk - 1 > (n - 1) / block)
        return fail(PSS_EINVAL, "rfi_clean: nblk %lld blocks of %lld samples start beyond n %lld", (long long)nblk,
                    (long long)block, (long long)n);
    const bool inplace = (const float *)out == data && out_ld == ld;
    if (!inplace) {
        const uintptr_t d0 = (uintptr_t)data, d1 = d0 + ((uintptr_t)(nchan - 1) * (uintptr_t)ld + (uintptr_t)n) * 4;
        const uintptr_t o0 = (uintptr_t)out, o1 = o0 + ((uintptr_t)(nchan - 1) * (uintptr_t)out_ld + (uintptr_t)n) * 4;
        if (d0 < o1 && o0 < d1)
            return fail(PSS_EINVAL, "rfi_clean: out and data overlap (in place takes out == data and out_ld == ld)");
    }
    const dim3 grid = grid_1d("rfi_clean", (n + kRfTile - 1) / kRfTile, "time tiles", 1, "channel group");
    if (!grid.x) return PSS_EINVAL;
    RfArgs a;
    a.n = n; a.ld = ld; a.out_ld = out_ld; a.block = block; a.nblk = nblk;
    a.nchan = nchan; a.per = (nchan + kRfQ - 1) / kRfQ; a.inplace = inplace ? 1 : 0;
    const hipStream_t st = (hipStream_t)stream;
    // 16-B loads / stores need the rows on the 16-B grid.  Same bits.
    const bool vin = on_grid16(data, ld), vout = on_grid16(out, out_ld);
    if (vin && vout) rf_launch<true, true>(grid, st, zero_dm, data, mask, base, rgood, out, zser, a);
    else if (vin) rf_launch<true, false>(grid, st, zero_dm, data, mask, base, rgood, out, zser, a);
    else if (vout) rf_launch<false, true>(grid, st, zero_dm, data, mask, base, rgood, out, zser, a);
    else rf_launch<false, false>(grid, st, zero_dm, data, mask, base, rgood, out, zser, a);
    LAUNCHCHK();
    return PSS_OK;
}

}  // extern "C"
