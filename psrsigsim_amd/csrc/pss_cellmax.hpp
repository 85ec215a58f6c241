#pragma once
// pss_cellmax.hpp -- what the two searches of the DM-time plane share on the
// device (pss_boxsearch.hip: level = width, entry = start time;
// pss_harmsum.hip: level = harmonics, entry = bin): the coefficient a_k of a
// level, the total order of the candidates and the reduction of a workgroup's
// tile to one (z, code) per cell.  A fix to the tie rule or to the cross-wave
// path is made here, once.
#include "pss_common.hpp"

namespace pss {

static constexpr int kCmThreads = 256;
static constexpr int kCmOwn = 8;                          // tile entries per lane
static constexpr int kCmTile = kCmThreads * kCmOwn;       // tile entries per workgroup

// a_k = 2^(-k/2) = 2^-ceil(k/2) * (k odd ? fp32(sqrt 2) : 1): exact scalings of 0x3FB504F3
__device__ __forceinline__ float cm_coef(int k) {
    const float s = (k & 1) ? __uint_as_float(0x3FB504F3u) : 1.0f;
    return s * __uint_as_float((uint32_t)(127 - ((k + 1) >> 1)) << 23);
}

// "a beats b": larger z, then the smaller code (lower level, then earlier entry)
__device__ __forceinline__ bool cm_better(float za, int ca, float zb, int cb) {
    return za > zb || (za == zb && ca < cb);
}

// The cells of a tile.  Thread tid of the 256 holds the best (bz[i], bl[i]) --
// z and its level -- of the tile entries tid + 256 i, i < 8.  (z, code) of the
// 2048 entries go to LDS (wz, wcode: kCmTile each, 16-B aligned, free to be
// overwritten -- the caller has synchronised after their last use), code =
// level << 16 | entry - q cell.  Thread tid then scans the 8 consecutive
// entries 8 tid .. 8 tid + 7 (one cell holds them all: cell is a multiple of
// 16), and cell / 8 neighbouring threads combine by a butterfly of wave
// shuffles -- for cell >= 1024 across the waves as well, through redz / redc
// (one entry per wave) -- under cm_better.  One thread per cell stores z and
// code (0 where the cell holds no candidate, z = -inf) as dwords at cell
// q0 + (the tile's cell) of row j of snr / code (rows of out_ld cells), if
// that is below nq <= out_ld.  cell = 1 << lcell, a power of two in [16,
// kCmTile]; every branch on it is uniform.  All 256 threads call it.  (j and
// the matrices rather than the row pointers: the form that leaves every
// instantiation's registers as they were.)
__device__ __forceinline__ void cm_reduce_store(float *wz, int *wcode, float *redz, int *redc,
                                                const float (&bz)[kCmOwn], const int (&bl)[kCmOwn], int tid, int cell,
                                                int lcell, int64_t q0, int64_t nq, int j, int64_t out_ld,
                                                float *__restrict__ snr, int32_t *__restrict__ code) {
    const int cmask = cell - 1;
#pragma unroll
    for (int i = 0; i < kCmOwn; ++i) {
        const int e = tid + i * kCmThreads;
        wz[e] = bz[i];
        wcode[e] = (bl[i] << 16) | (e & cmask);
    }
    __syncthreads();
    float rz;
    int rc;
    {
        const float4 z0 = *reinterpret_cast<const float4 *>(wz + 8 * tid);
        const float4 z1 = *reinterpret_cast<const float4 *>(wz + 8 * tid + 4);
        const int4 c0 = *reinterpret_cast<const int4 *>(wcode + 8 * tid);
        const int4 c1 = *reinterpret_cast<const int4 *>(wcode + 8 * tid + 4);
        const float zz[8] = {z0.x, z0.y, z0.z, z0.w, z1.x, z1.y, z1.z, z1.w};
        const int cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
        rz = zz[0];
        rc = cc[0];
#pragma unroll
        for (int i = 1; i < 8; ++i)
            if (cm_better(zz[i], cc[i], rz, rc)) {
                rz = zz[i];
                rc = cc[i];
            }
    }
    const int tpc = cell >> 3;                             // threads per cell: 2 .. 256
    for (int off = 1; off < min(tpc, 64); off <<= 1) {
        const float oz = __shfl_xor(rz, off);
        const int oc = __shfl_xor(rc, off);
        if (cm_better(oz, oc, rz, rc)) {
            rz = oz;
            rc = oc;
        }
    }
    int qc = tid >> (lcell - 3);                           // the tile's cell of this thread
    bool writer = (tid & (tpc - 1)) == 0;
    if (tpc > 64) {                                        // (uniform) cell 1024 or 2048: across the waves
        if ((tid & 63) == 0) {
            redz[tid >> 6] = rz;
            redc[tid >> 6] = rc;
        }
        __syncthreads();
        const int wpc = tpc >> 6;                          // waves per cell: 2 or 4
        writer = tid < kCmThreads / tpc;
        qc = tid;
        if (writer) {
            rz = redz[tid * wpc];
            rc = redc[tid * wpc];
            for (int w = 1; w < wpc; ++w) {
                const float oz = redz[tid * wpc + w];
                const int oc = redc[tid * wpc + w];
                if (cm_better(oz, oc, rz, rc)) {
                    rz = oz;
                    rc = oc;
                }
            }
        }
    }
    const int64_t q = q0 + qc;
    if (writer && q < nq) {
        PSS_DASSERT(q >= 0 && q < out_ld);
        snr[(int64_t)j * out_ld + q] = rz;
        code[(int64_t)j * out_ld + q] = rz == -INFINITY ? 0 : rc;
    }
}

}  // namespace pss
