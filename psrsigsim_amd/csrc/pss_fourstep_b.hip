// pss_fourstep_b.hip -- the power-of-two four-step lengths other than C3's 2^22
// (2^14 .. 2^21, 2^23, 2^24), compiled in parallel with pss_fourstep.hip.
#include "pss_fourstep.hpp"

using namespace pss;

int run_fourstep_b(KP &k, hipStream_t st, const float *mask_row) {
    // k.N1 x k.N2: fourstep_split (set by run_fourstep)
    if (k.N2 == 16384 && k.N1 == 1024) {
        // C5 (2^24, a plain delay): C3's column kernels (1024-point columns:
        // pass A two workgroups per CU, pass C 16-column blocks) and a
        // one-row-at-a-time 16384-point row pass (PairRowsSeq, 1024
        // threads, 133 KB of LDS)
        return launch_pair<1024, 8, 512, C1kF, C1kF, 16384, 1024, C16kF, C16kI, 1024, kBC, kTC>(k, st, mask_row);
    }
    if (k.N2 == 8192) {
        switch (k.N1) {
            case 1024:   // 2^23
                return launch_pair<1024, 8, 512, C1kF, C1kF, 8192, 1024, C8kF, C8kI, 512>(k, st, mask_row);
            case 2048:
                // 2^24 with a delayed null, a transfer function or the tail.
                // Pass A: the LDS-staged fast kernel on 2048-point columns;
                // pass C: 16-column register-resident blocks (passC_fast32)
                return launch_pair<2048, 8, 512, C2kF, C2kF, 8192, 1024, C8kF, C8kI, 512, 8, 1024>(k, st, mask_row);
            default: break;
        }
    } else if (k.N1 == 16) {
        // 2^14 .. 2^16: 16 columns, rows of N / 16
        switch (k.N2) {
            case 1024:
                return launch_pair<16, 512, 512, C16, C16, 1024, 128, C1kF, C1kI, 64>(k, st, mask_row);
            case 2048:
                return launch_pair<16, 512, 512, C16, C16, 2048, 256, C2kF, C2kI, 128>(k, st, mask_row);
            case 4096:
                return launch_pair<16, 512, 512, C16, C16, 4096, 512, C4k, C4k, 256>(k, st, mask_row);
            default: break;
        }
    } else if (k.N2 == 4096) {
        // 2^17 .. 2^21: rows of 4096 (the C3 row kernel: two rows of a pair
        // in 66 KB, two workgroups per CU) and N / 4096 columns; the column
        // kernels keep their 8192 / N1-column blocks (N2 / B >= 16 per pair)
        switch (k.N1) {
#define CASE4K(N1_, CF, CI)                                                                          \
    case N1_:                                                                                        \
        return launch_pair<N1_, 8192 / N1_, 512, CF, CF, 4096, 512, C4k, C4k, 256>(k, st, mask_row);
            CASE4K(32, C32F, C32I)
            CASE4K(64, C64F, C64I)
            CASE4K(128, C128F, C128I)
            CASE4K(256, C256, C256)
            CASE4K(512, C512F, C512I)
#undef CASE4K
            default: break;
        }
    }
    return fail(PSS_EUNSUPPORTED, "four-step: %lld x %lld", (long long)k.N1, (long long)k.N2);
}
