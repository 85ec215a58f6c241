// pss_single.hip -- N = 2^m <= 8192: a row (or rows) per workgroup in LDS.
#include "pss_stages.hpp"
#include "pss_fft.hpp"

using namespace pss;

// ---------------------------------------------------------------------------
// path 1: whole row(s) in LDS.  BATCH rows of length L per workgroup.
// ---------------------------------------------------------------------------
template <int L, int BATCH, int T, typename FWD, typename INV>
struct SinglePass;

template <int L, int BATCH, int T, int... F, int... I>
struct SinglePass<L, BATCH, T, RList<F...>, RList<I...>> {
    using FF = Fft<L, BATCH, T>;
    static constexpr int E = FF::E;
    static constexpr int RF0 = FF::template first<F...>();
    static constexpr int RFL = FF::template last_of<F...>();
    static constexpr int RIL = FF::template last_of<I...>();
    static_assert(RIL == RF0, "inverse plan must be the reversed forward plan");

    __device__ static void body(const KP &k) {
        __shared__ cf lds[BATCH * Lds<L>::RS];
        const int tid = threadIdx.x;
        const int r0 = blockIdx.x * BATCH;
        const PssPipeline &p = k.p;
        const bool re_in = p.data_in_fft != 0;
        // source -> LDS
        for (int it = tid; it < BATCH * L / 4; it += T) {
            const int b = it / (L / 4);
            const int n0 = (it - b * (L / 4)) * 4;
            float re[4], im[4];
            if (r0 + b < p.nchan) source4(k, r0 + b, n0, 4, re, im, re_in);
            else { for (int i = 0; i < 4; ++i) { re[i] = 0.f; im[i] = 0.f; } }
#pragma unroll
            for (int i = 0; i < 4; ++i) lds[Lds<L>::at(b, n0 + i)] = make_float2(re[i], im[i]);
        }
        __syncthreads();
        cf v[E];
        FF::template load<RF0>(v, lds, tid);
        __syncthreads();
        FF::template run<false, 1, F...>(v, lds, tid);
        // ramp on natural-order spectrum (last forward stage mapping)
#pragma unroll
        for (int i = 0; i < E; ++i) {
            int b, pos;
            FF::template where<RFL>(i, tid, b, pos);
            const int rr = min(r0 + b, p.nchan - 1);
            v[i] = apply_ramp(k, rr, pos, v[i]);
        }
        FF::template run<true, 1, I...>(v, lds, tid);
        FF::template store<RIL>(v, lds, tid);
        __syncthreads();
        for (int it = tid; it < BATCH * L / 4; it += T) {
            const int b = it / (L / 4);
            const int n0 = (it - b * (L / 4)) * 4;
            if (r0 + b >= p.nchan) continue;
            float pre[4], msk[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                cf z = lds[Lds<L>::at(b, n0 + i)];
                pre[i] = z.x * k.invN;
                msk[i] = z.y * k.invN;
            }
            if (k.w1_out) {
                // (data, mask) for the float64 null refine; the epilogue runs
                // after it (k_fb_epilogue, as on the other packed paths)
                cf *w = k.w1_out + (int64_t)(r0 + b) * L + n0;
#pragma unroll
                for (int i = 0; i < 4; ++i) w[i] = make_float2(pre[i], msk[i]);
            } else {
                epilogue4(k, r0 + b, n0, 4, pre, msk, !re_in);
            }
        }
    }
};

template <typename SP, int T>
__global__ __launch_bounds__(T) void k_single(KP k) { SP::body(k); }

template <int L, int BATCH, int T, typename F, typename I>
static int launch_single(const KP &k, hipStream_t st) {
    using SP = SinglePass<L, BATCH, T, F, I>;
    dim3 grid((k.p.nchan + BATCH - 1) / BATCH);
    plan_note("single %d", L);
    tk_begin(TK_SINGLE, st);
    k_single<SP, T><<<grid, dim3(T), 0, st>>>(k);
    tk_end(st);
    LAUNCHCHK();
    return PSS_OK;
}

static int launch_single_n(KP &k, hipStream_t st) {
    switch (k.N) {
        case 64: return launch_single<64, 64, 256, C64F, C64I>(k, st);
        case 128: return launch_single<128, 32, 256, C128F, C128I>(k, st);
        case 256: return launch_single<256, 16, 256, C256, C256>(k, st);
        case 512: return launch_single<512, 8, 256, C512F, C512I>(k, st);
        case 1024: return launch_single<1024, 4, 256, C1kF, C1kI>(k, st);
        case 2048: return launch_single<2048, 2, 256, C2kF, C2kI>(k, st);
        case 4096: return launch_single<4096, 1, 256, C4k, C4k>(k, st);
        case 8192: return launch_single<8192, 1, 512, C8kF, C8kI>(k, st);
        default: break;
    }
    return fail(PSS_EUNSUPPORTED, "single-pass: N=%lld", (long long)k.N);
}

int run_single(KP &k, hipStream_t st) {
    k.N1 = 1;
    k.N2 = k.N;
    if (!refine_null(k)) return launch_single_n(k, st);
    // a delayed null decided in float64: the kernel leaves
    // (data, mask) per sample in W1, the samples within the fp32 error of the
    // threshold are re-decided from the box row's float64 spectrum
    // (launch_null_refine), then the epilogue (null, observe copy, noise, store)
    k.w1_out = reinterpret_cast<cf *>(k.p.work);
    int rc = launch_single_n(k, st);
    if (!rc) rc = launch_null_refine(k, st);
    if (!rc) rc = launch_fb_epilogue(k, st);
    return rc;
}

