// pss_fourstep_b.hip -- the power-of-two four-step lengths other than C3's 2^22
// (2^14 .. 2^21, 2^23, 2^24), compiled in parallel with pss_fourstep.hip.
#include "pss_fourstep.hpp"

using namespace pss;

static constexpr int64_t split_key(int64_t n1, int64_t n2) { return (n1 << 32) | n2; }

int run_fourstep_b(KP &k, hipStream_t st, const float *mask_row) {
    // k.N1 x k.N2: fourstep_split (set by run_fourstep)
    switch (split_key(k.N1, k.N2)) {
        // 2^14 .. 2^16: 16 columns, rows of N / 16
        case split_key(16, 1024): return launch_pair<Pow2Split<16, 1024>>(k, st, mask_row);
        case split_key(16, 2048): return launch_pair<Pow2Split<16, 2048>>(k, st, mask_row);
        case split_key(16, 4096): return launch_pair<Pow2Split<16, 4096>>(k, st, mask_row);
        // 2^17 .. 2^21: rows of 4096 (the C3 row kernel: two rows of a pair
        // in 66 KB, two workgroups per CU) and N / 4096 columns; the column
        // kernels keep their 8192 / N1-column blocks (N2 / B >= 16 per pair)
        case split_key(32, 4096): return launch_pair<Pow2Split<32, 4096>>(k, st, mask_row);
        case split_key(64, 4096): return launch_pair<Pow2Split<64, 4096>>(k, st, mask_row);
        case split_key(128, 4096): return launch_pair<Pow2Split<128, 4096>>(k, st, mask_row);
        case split_key(256, 4096): return launch_pair<Pow2Split<256, 4096>>(k, st, mask_row);
        case split_key(512, 4096): return launch_pair<Pow2Split<512, 4096>>(k, st, mask_row);
        // 2^23
        case split_key(1024, 8192): return launch_pair<Pow2Split<1024, 8192>>(k, st, mask_row);
        // 2^24 with a delayed null, a transfer function or the tail.
        // Pass A: the LDS-staged fast kernel on 2048-point columns;
        // pass C: 16-column register-resident blocks (passC_fast32)
        case split_key(2048, 8192): return launch_pair<Pow2Split<2048, 8192>>(k, st, mask_row);
        // C5 (2^24, a plain delay): C3's column kernels (1024-point columns:
        // pass A two workgroups per CU, pass C 16-column blocks) and a
        // one-row-at-a-time 16384-point row pass (PairRowsSeq, 1024
        // threads, 133 KB of LDS)
        case split_key(1024, 16384): return launch_pair<Pow2Split<1024, 16384>>(k, st, mask_row);
        default: return fail(PSS_EUNSUPPORTED, "four-step: %lld x %lld", (long long)k.N1, (long long)k.N2);
    }
}
