#pragma once
// pss_common.hpp -- what every unit of the library needs and nothing else:
// error reporting, the launch checks and the small host / device helpers the
// stand-alone stages (pss_searchout, pss_channelize, pss_dedisperse,
// pss_boxsearch, pss_harmsum, pss_foldseries) share with the synthesis engine.
// See include/pss_hip.h for the ABI.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pss_device.hpp"
#include "../../include/pss_hip.h"

// ---------------------------------------------------------------------------
// error reporting (defined in pss_pipeline.hip)
// ---------------------------------------------------------------------------
int fail(int code, const char *fmt, ...);

#define HIPCHK(x)                                                              \
    do {                                                                       \
        hipError_t e_ = (x);                                                   \
        if (e_ != hipSuccess)                                                  \
            return fail(PSS_EHIP, "%s: %s", #x, hipGetErrorString(e_));        \
    } while (0)

#define LAUNCHCHK()                                                            \
    do {                                                                       \
        hipError_t e_ = hipGetLastError();                                     \
        if (e_ != hipSuccess)                                                  \
            return fail(PSS_EHIP, "launch failed: %s", hipGetErrorString(e_)); \
    } while (0)

static inline bool is_pow2(int64_t n) { return n > 0 && (n & (n - 1)) == 0; }

static inline int64_t al256(int64_t b) { return (b + 255) & ~255ll; }

static inline dim3 stream_grid(int64_t items, int rows) {
    int64_t bx = (items + 255) / 256;
    if (bx > 4096) bx = 4096;
    if (bx < 1) bx = 1;
    return dim3((unsigned)bx, (unsigned)rows, 1);
}

// rows of pitch ld (floats) from p on the 16-B grid: every row start, and every
// fourth sample of a row, may be moved as a float4
static inline bool on_grid16(const void *p, int64_t ld) { return (uintptr_t)p % 16 == 0 && ld % 4 == 0; }

// The 1-D grid of na x nb workgroups (both >= 1) of a stage whose kernel maps
// blockIdx.x through xcd_run_id; the product must fit 2^31 - 1.  On failure
// the error is recorded ("<stage>: <na> <a> x <nb> <b> exceed ...") and the
// grid returned is empty: `if (!grid.x) return PSS_EINVAL;`.
static inline dim3 grid_1d(const char *stage, int64_t na, const char *a, int64_t nb, const char *b) {
    if (na > (int64_t)0x7fffffff / nb) {
        fail(PSS_EINVAL, "%s: %lld %s x %lld %s exceed 2^31 - 1 workgroups", stage, (long long)na, a, (long long)nb, b);
        return dim3(0);
    }
    return dim3((unsigned)(na * nb));
}

// the cell of a per-cell reduction (pss_cellmax.hpp): a power of two in [16, tile]
static inline int check_cell(const char *stage, int32_t cell, int tile) {
    if (cell < 16 || cell > tile || (cell & (cell - 1)))
        return fail(PSS_EINVAL, "%s: cell %d is not a power of two in [16, %d]", stage, cell, tile);
    return PSS_OK;
}

static inline int32_t cell_log2(int32_t cell) {
    int32_t l = 0;
    while ((1 << l) < cell) ++l;
    return l;
}

// Logical id of workgroup blockIdx.x of a 1-D grid under the "contiguous runs
// per XCD" map: workgroup ids are dealt to the 8 XCDs round-robin, so XCD x is
// given the contiguous run of logical ids [x base + min(x, rem), ..) (base =
// total / 8, rem = total % 8; any grid size).  Neighbouring logical ids then
// run on one XCD, side by side, and share its L2.  Placement only changes the
// speed.  (xcd_block, pss_stages.hpp, is the column passes' own 2-D map.)
__device__ __forceinline__ unsigned xcd_run_id() {
    const unsigned total = gridDim.x, base = total >> 3, rem = total & 7u;
    const unsigned xcd = blockIdx.x & 7u;
    return xcd * base + min(xcd, rem) + (blockIdx.x >> 3);
}

// ... as (slow, fast) indices of a grid of nslow x nfast workgroups, the fast
// index running fastest: the nfast workgroups of one slow index run side by
// side on one XCD
__device__ __forceinline__ uint2 xcd_run_pair(unsigned nfast) {
    const unsigned lid = xcd_run_id();
    return make_uint2(lid / nfast, lid % nfast);
}
