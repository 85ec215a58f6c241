#pragma once
// pss_window.hpp -- the copy of a row's window into LDS, shared by the stages
// that gather from one (pss_dedisperse.hip: float samples; pss_accel.hip: the
// same words moved as bits).  Include after pss_common.hpp.
#include "pss_common.hpp"

namespace pss {

template <typename W> struct Word4;
template <> struct Word4<float> { typedef float4 type; };
template <> struct Word4<uint32_t> { typedef uint4 type; };

// row[wb .. wb + need) -> w[0 .. need) by the THREADS threads of a workgroup,
// as nq = ceil(need / 4) <= WIN / 4 whole 16-B groups (w holds WIN words).
// Where VEC holds, row + wb is on the 16-B grid of the address.  HEAD: the
// window may begin up to 3 words before the row (wb >= -3: a row that begins
// off the grid); without it wb >= 0 is the caller's promise and costs no
// compare.  Words outside [0, n) of the row are never needed and are zeros.
//   fast    (VEC && wb >= 0 && wb + 4 nq <= n: every group inside the row):
//           16-B loads.  The loads of all passes are issued, unconditionally,
//           before the first LDS store waits for one -- a load-store loop pays
//           one global latency per pass -- and pinned there by an empty asm,
//           or each load sinks into the branch of its store.  The lanes past
//           the last group re-load it (in bounds, one cache line for all of
//           them); a pass with work stores every lane's value, the copies in
//           slots of the window that nothing reads.
//   element (otherwise: rows off the grid, and a window whose head or tail
//           leaves the row by part of a group): bounded element loads -- the
//           same values in the same words.
template <int THREADS, int WIN, bool VEC, bool HEAD, typename W>
__device__ __forceinline__ void stage_window(W *w, const W *row, int64_t wb, int need, int64_t n, int tid) {
    typedef typename Word4<W>::type W4;
    static_assert(WIN % (4 * THREADS) == 0, "whole passes of 16-B loads");
    PSS_DASSERT(need >= 1 && need <= WIN && wb >= (HEAD ? -3 : 0) && wb + need <= n);
    const int nq = (need + 3) >> 2;
    if (VEC && (!HEAD || wb >= 0) && wb + 4 * (int64_t)nq <= n) {
        constexpr int NP = WIN / 4 / THREADS;
        const W4 *src = reinterpret_cast<const W4 *>(row + wb);
        W4 v[NP];
#pragma unroll
        for (int i = 0; i < NP; ++i) v[i] = src[min(tid + i * THREADS, nq - 1)];
#pragma unroll
        for (int i = 0; i < NP; ++i) asm volatile("" : "+v"(v[i].x), "+v"(v[i].y), "+v"(v[i].z), "+v"(v[i].w));
#pragma unroll
        for (int i = 0; i < NP; ++i)
            if (i * THREADS < nq) *reinterpret_cast<W4 *>(w + 4 * (tid + i * THREADS)) = v[i];
        return;
    }
    for (int q = tid; q < nq; q += THREADS) {
        const int64_t s = wb + 4 * q;
        W4 v;
        v.x = (!HEAD || s >= 0) && s < n ? row[s] : W(0);
        v.y = (!HEAD || s + 1 >= 0) && s + 1 < n ? row[s + 1] : W(0);
        v.z = (!HEAD || s + 2 >= 0) && s + 2 < n ? row[s + 2] : W(0);
        v.w = (!HEAD || s + 3 >= 0) && s + 3 < n ? row[s + 3] : W(0);
        *reinterpret_cast<W4 *>(w + 4 * q) = v;
    }
}

}  // namespace pss
