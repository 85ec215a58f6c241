/*
 * pss_hip.h -- C ABI of libpss_hip.so, the MI355X (gfx950) engine behind
 * PsrSigSim's filterbank synthesis path.
 *
 * The reference has no FFI: its boundary is the Python method API (SURVEY.md
 * §8(b)).  Each entry point below replaces one reference call (or a fused run
 * of several), cited file:line against /root/reference/psrsigsim.  The Python
 * layer (psrsigsim_amd, ctypes) mirrors the reference classes and calls these.
 *
 * Conventions
 *  - All buffers are DEVICE pointers owned by the caller (torch); the library
 *    never allocates or frees user memory.  Row-major [chan][sample] fp32.
 *  - Every call is stream-ordered on `stream` (a hipStream_t; NULL = default)
 *    and performs no host synchronisation; it is graph-capturable.
 *  - Return codes: PSS_OK = 0, PSS_EINVAL = -1 (-> ValueError),
 *    PSS_EUNSUPPORTED = -2 (-> NotImplementedError), PSS_EHIP = -3
 *    (-> RuntimeError); pss_last_error() returns the message.
 *  - Randomness is counter-based Philox4x32-7 keyed by (seed, call id,
 *    purpose, GLOBAL channel, sample): results do not depend on how channels
 *    are split across launches or GPUs.
 */
#ifndef PSS_HIP_H
#define PSS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSS_OK 0
#define PSS_EINVAL (-1)
#define PSS_EUNSUPPORTED (-2)
#define PSS_EHIP (-3)

/* source of the real (data) part */
#define PSS_SRC_LOAD 0   /* read `data` (an already materialised signal)       */
#define PSS_SRC_SEARCH 1 /* pulsar.py:222-244 PCHIP(phase) x chi2(df) x norm    */
#define PSS_SRC_FOLD 2   /* pulsar.py:196-221 tile(profile) x chi2(Nfold) x norm */

/* null stage */
#define PSS_NULL_NONE 0
#define PSS_NULL_UNDELAYED 1 /* pulsar.py:292-304: replace boxes, shared vector  */
#define PSS_NULL_DELAYED 2   /* pulsar.py:306-330: chi2(100) box mask shifted
                                through the same FFT, thresholded > 1           */

/* observe() copy ("out") dtypes */
#define PSS_OUT_NONE 0
#define PSS_OUT_F32 1
#define PSS_OUT_I8 2

/*
 * One fused run of the synthesis path over `nchan` rows:
 *
 *   source  ->  [delay ramp: rfft -> exp(-2 pi i f tau) -> irfft]  ->  [null]
 *           ->  [radiometer noise]  ->  data      (+ optional pre-noise `out`)
 *
 * Replaces, for one signal, the sequence
 *   Pulsar.make_pulses        pulsar/pulsar.py:107-151,185-244
 *   ISM.disperse / FD_shift / scatter_broaden(convolve=False)
 *                             ism/ism.py:20-74, 100-156, 158-220
 *                             (each = per-channel utils.shift_t, utils/utils.py:17-59)
 *   Pulsar.null               pulsar/pulsar.py:246-333
 *   Telescope.observe (copy branch) + Receiver.radiometer_noise
 *                             telescope/telescope.py:72-149, receiver.py:82-172
 * with any prefix/subset of the stages enabled.  Several delay stages are
 * fused into one forward/inverse FFT pair: phase exp(-2 pi i k sum(s_j)/N) on
 * every bin, and on the Nyquist bin the product of the per-stage factors
 * cos(pi s_j) that the reference's irfft imposes.
 */
typedef struct PssPipeline {
    /* geometry */
    int32_t nchan;      /* rows in this launch                                  */
    int32_t chan0;      /* global channel index of row 0 (RNG key, table rows)  */
    int64_t nsamp;      /* N: samples per row (= data.shape[1])                */
    int64_t ld;         /* row stride of `data` in elements                     */
    float *data;        /* [nchan][ld] in/out                                   */
    void *work;         /* workspace, >= pss_workspace_bytes(nchan, nsamp)      */

    /* source */
    int32_t src;        /* PSS_SRC_*                                            */
    int32_t prof_rows;  /* rows of `prof` (1 = same profile for every channel)  */
    const float *prof;  /* SEARCH: [prof_rows][nint][4] PCHIP coefficients in the
                           local interval coordinate u in [0,1): c3 u^3+c2 u^2+c1 u+c0
                           FOLD: [prof_rows][nph] profile samples              */
    int32_t nint;       /* SEARCH: number of PCHIP intervals                    */
    int32_t nph;        /* FOLD: phase bins per period; NULL: box length        */
    uint64_t phase_step;/* SEARCH: 2^64 / (samples per period), i.e. the pulse
                           phase advance per sample in 2^-64 cycles             */
    uint32_t knot_m;    /* SEARCH: 1/knot spacing (intervals per cycle)         */
    float gen_df;       /* chi2 degrees of freedom of the pulse draws           */
    float draw_norm;    /* signal._draw_norm                                    */

    /* delay ramp (fused delay stages) -- all arrays indexed by local row       */
    int32_t shift;          /* 1: run the FFT delay engine                     */
    int32_t data_in_fft;    /* 1: real part carries the data through the FFT;
                               0: the epilogue reads `data` unshifted (only the
                               null mask goes through the FFT)                  */
    const uint64_t *ramp;   /* [nchan] frac(s/N) in 2^-64 cycles, s = total delay
                               in samples: bin k gets exp(-2 pi i k' s / N)     */
    const float *nyq_re;    /* [nchan] Nyquist factor for the real part         */
    const float *nyq_im;    /* [nchan] Nyquist factor for the imaginary part    */

    /* null */
    int32_t null_mode;      /* PSS_NULL_*                                       */
    int32_t null_slots;     /* length of null_rank (= nsub)                     */
    const int32_t *null_rank;  /* [null_slots] order of the nulled pulse in the
                               reference's np.random.choice list, or -1         */
    int64_t null_shift;     /* shift_val (pulsar.py:286)                        */
    float null_box_df;      /* chi2 df of the box values (mask / undelayed)     */
    float null_box_scale;   /* box scale: draw_norm (mask) or draw_norm*opm     */
    float null_rep_df;      /* DELAYED: df of the replacement draws             */
    float null_rep_scale;   /* DELAYED: draw_norm * off-pulse mean              */

    /* radiometer noise */
    int32_t noise;          /* 1: data += noise_norm * chi2(noise_df)           */
    float noise_df;
    float noise_norm;

    /* observe() pre-noise copy */
    int32_t out_kind;       /* PSS_OUT_*                                        */
    void *out;              /* [nchan][nsamp] float32 or int8                   */
    float clip;             /* out = min(pre-noise, clip) (telescope.py:140-145)*/

    /* randomness */
    uint64_t seed;
    uint32_t call_gen;      /* call ids: one per API call that drew randomness  */
    uint32_t call_null;     /* (make_pulses / null / noise), so that repeated   */
    uint32_t call_noise;    /* calls draw fresh values, like np.random          */

    /* exact mode: injected draws (NULL = use Philox) */
    const float *inj_gen;     /* [nchan][nsamp] pulse chi2 draws                */
    const float *inj_box;     /* [nsamp] box values (already scaled), shared    */
    const float *inj_rep;     /* [nchan][nsamp] DELAYED replacement values      */
    const float *inj_noise;   /* [nchan][nsamp] noise chi2 draws                */

    /* DELAYED null: [nchan] frac(s_mask/N) in 2^-64 cycles, s_mask = the
       signal's total delay in samples (pulsar.py:322-325).  Four-step lengths
       (N = 2^m >= 2^14) decide mask > 1 from a once-per-run table of the box
       row shifted by the fraction of s_mask; the other
       lengths use `ramp`/`nyq_im` and carry the mask through the FFT.       */
    const uint64_t *mask_ramp;

    /* Baseband path (ISM._disperse_baseband ism/ism.py:76-98,
       Pulsar._make_amp_pulses pulsar/pulsar.py:153-183).                     */
    int32_t gen_amp;        /* SEARCH source: sqrt(profile) x N(0,1) draws
                               (amplitude pulses) instead of profile x chi2;
                               1: PCHIP table, 2: analytic Gaussians, prof =
                               [nint][4] {peak, 1/width, amp/Amax, 0} and
                               knot_m = 1 (portraits.py:277-290)             */
    int32_t prof_row0;      /* global channel of `prof`'s row 0 when the table
                               holds a channel window (shard-local planning):
                               channel c reads row c - prof_row0; 0 for a
                               band-wide table (ignored when prof_rows == 1)  */
    const float *htab;      /* [nsamp/2 + 1] complex64 transfer function H(k)
                               of the reference's rfft bins (same for every
                               row): bin k gets H(k), bin N-k conj H(k), DC
                               and Nyquist Re H (irfft drops their imaginary
                               parts).  Non-NULL: replaces the delay ramp and
                               takes the direct / Bluestein transforms.      */
    const int64_t *null_shift_dev;  /* NULL: use null_shift; else the device
                               word pss_null_shift wrote (shift_val computed on
                               the device, no host round trip)                */
    const float *tail_a;    /* [nchan] scattering tail (extension, no reference
                               counterpart -- SURVEY App. A.11): circular
                               convolution of each row with the normalised
                               exponential h[n] = (1-a) a^n, a = exp(-dt/tau_c),
                               i.e. bin k x H(k) = (1-a) / (1 - a e^{-2 pi i k/N})
                               in the same forward/inverse pass as the delay
                               ramp; NULL = none                             */
    int32_t prof_split;     /* SEARCH: 1 = `prof` holds split cells for a portrait
                               on non-uniform phases: [prof_rows][nint][8]
                               (the cubics left and right of the cell's one
                               interior knot, in the cell coordinate u) followed
                               by [nint] split points (u >= split: right cubic;
                               2 = no knot in the cell); knot_m = nint cells */
    /* observe()'s RESAMPLED pre-noise copy, produced by the run itself
       (telescope.py:108-125 down_sample / rebin, then :140-145 clip and cast):
       out_len > 0 makes `out` [nchan][out_len] of kind out_kind, bin i = the
       mean of the pre-noise samples [lo_i, hi_i), clipped from above at `clip`.
       Every epilogue adds its samples' values into out_acc (float64 window
       sums, zeroed by pss_run), a final small kernel divides, clips and casts:
       no full-resolution copy, no separate resampling pass.                 */
    int32_t out_len;        /* 0: `out` is the full [nchan][nsamp] copy         */
    const int64_t *out_lo;  /* [out_len] window starts (utils.py:77-89's ceil
                               edges), or NULL: uniform windows of out_step
                               samples, lo_i = i * out_step (down_sample,
                               utils.py:62-68)                                 */
    const int64_t *out_hi;  /* [out_len] window ends (exclusive), or NULL       */
    double out_step;        /* nominal window width: the bin of sample n is
                               floor(n / out_step) or the one before it; an
                               integer >= 1 when out_lo is NULL               */
    double *out_acc;        /* [nchan][out_len] float64 scratch                 */
} PssPipeline;

/* Library / device info. */
int pss_version(void);
/* "PSS_BUILD_HASH=<sha256 of the sources the library was built from>". */
const char *pss_build_hash(void);

/* Engine flags (test hook; returns the previous flags).  PSS_FLAG_NO_FAST
 * routes every run through the generic kernels instead of the fast-path
 * specialisations (which must give bitwise identical results). */
#define PSS_FLAG_NO_FAST 1
/* PSS_FLAG_DIRECT_DFT sends the fallback lengths N > 8192 through the O(N^2)
 * direct DFT instead of the Bluestein (chirp-z) path (test hook). */
#define PSS_FLAG_DIRECT_DFT 2
/* PSS_FLAG_NULL_F32 keeps the packed (direct / Bluestein) paths' delayed-null
   decisions in fp32 (no float64 re-evaluation near the threshold).          */
#define PSS_FLAG_NULL_F32 4
/* PSS_FLAG_REFINE_PER_SAMPLE runs those float64 re-evaluations through the
   per-sample kernel instead of the compacted candidate list (the list's
   overflow path; test hook: both give the same bits).                      */
#define PSS_FLAG_REFINE_PER_SAMPLE 8
int pss_set_flags(int flags);
int pss_last_error(char *buf, size_t n);

/* Launch-plan log (test hook): the kernels every pss_run since the last call
 * picked, one line per run -- "<nchan>x<nsamp>: <path> <split> A:<pass A>
 * R:<row pass> C:<pass C> N:<null>", e.g. "2048x4194304: fourstep 1024x4096
 * A:fast R:pair_row C:fast N:table N:fix_list" -- copied into buf (up to n - 1
 * bytes, NUL-terminated); returns the log's length and clears it.  The parity
 * tests assert with it which kernels produced the bits they check.  "C:null"
 * (after "C:fast C:cols16x2", a delayed null on 1024-point columns): pass C
 * nulled the samples the mask table nulls for every fractional shift itself,
 * and "N:fix_list" then rewrites only the f-dependent hits.                */
int pss_plan_collect(char *buf, size_t n);

/* Opt-in kernel timing for benchmarks: while enabled, pss_run records a pair
 * of hipEvents on its stream around every kernel it launches.  collect()
 * synchronises on them and returns, per launch (up to `cap`), the kernel kind
 * (0 elementwise, 1 single pass, 2 four-step column pass A, 3 row pass B,
 * 4 column pass C, 5 fallback, 6 delayed-null fix-up), its milliseconds and the channel-samples it
 * processed; returns the number of launches reported and resets. */
void pss_timing_enable(int on);
int pss_timing_collect(int32_t *kind, double *ms, int64_t *units, int cap);
/* Milliseconds from the start of the first timed launch to the end of the
 * last one since the last collect (the device span of the runs: with pair
 * batches on side streams the per-kernel times overlap). */
double pss_timing_span_ms(void);

/* Workspace bytes the fused run needs for `nchan` rows of length `nsamp`. */
int64_t pss_workspace_bytes(int32_t nchan, int64_t nsamp);

/* The FFT plan a delay-stage run of `nsamp` samples per row takes (host only,
 * no GPU touched): returns its kind and writes the geometry to n1 x n2
 * (either may be NULL) --
 *   SINGLE      one workgroup per row(s), 2^m in [64, 8192]: 1 x nsamp
 *   FOURSTEP    power-of-two four-step: columns x rows (N1 x N2)
 *   SMOOTH      mixed-radix four-step: N1 x N2
 *   DIRECT      O(N^2) direct DFT: 0 x 0 (no split)
 *   BLUESTEIN   chirp-z through an M1 x M2 power-of-two four-step
 *   UNSUPPORTED odd or non-positive nsamp, other lengths above 2^24
 * `variant`: 0 a delay only, 1 with a delayed null (null_mode
 * PSS_NULL_DELAYED), 2 with a transfer function or the scattering tail (htab
 * / tail_a) and no delayed null.  Honours PSS_FLAG_DIRECT_DFT.  These are
 * the functions pss_run's launchers take their split from. */
#define PSS_PLAN_UNSUPPORTED 0
#define PSS_PLAN_SINGLE 1
#define PSS_PLAN_FOURSTEP 2
#define PSS_PLAN_SMOOTH 3
#define PSS_PLAN_DIRECT 4
#define PSS_PLAN_BLUESTEIN 5
int pss_plan_geometry(int64_t nsamp, int32_t variant, int64_t *n1, int64_t *n2);

/* The fused run (see PssPipeline). */
int pss_run(const PssPipeline *p, void *stream);

/*
 * utils.shift_t on a batch of rows (utils/utils.py:17-59): every row r is
 * shifted by shift_samples[r] (= shift/dt, may be fractional) through the same
 * FFT engine.  `nyq` is the Nyquist factor per row (cos(pi*s) for one
 * reference call; unused for odd N).  In place.  Odd N (3 <= N <= 2^20): the
 * reference's irfft without n= returns N-1 samples (utils.py:57); they are
 * written to the first N-1 columns of each row (direct DFTs, f64 sums).
 */
/* Filter rows by a per-bin transfer function (baseband coherent dispersion,
 * ism/ism.py:76-98): rows <- irfft(rfft(row) * H) in place, H = htab
 * [n/2 + 1] complex64 (interleaved re, im).  Even n <= 2^24.  Workspace:
 * pss_filter_workspace_bytes(nrows, n). */
int64_t pss_filter_workspace_bytes(int32_t nrows, int64_t n);
int pss_filter_rows(float *rows, int32_t nrows, int64_t n, int64_t ld, const float *htab,
                    void *work, void *stream);

int pss_shift_rows(float *rows, int32_t nrows, int64_t n, int64_t ld,
                   const uint64_t *ramp, const float *nyq, void *work, void *stream);

/* utils.down_sample per row (utils/utils.py:62-68): out[r][i] = mean of
 * in[r][i*fact : (i+1)*fact]; in_len must be a multiple of fact. */
int pss_down_sample(const float *in, float *out, int32_t nrows, int64_t in_len,
                    int64_t in_ld, int32_t fact, void *stream);

/* utils.rebin per row (utils/utils.py:71-91): `lo`/`hi` are the integer window
 * edges [lo_i, hi_i) the reference derives from its ceil() arithmetic, device
 * arrays of `newlen` entries with 0 <= lo_i <= hi_i <= in_len (not checked:
 * they live on the device).  PSS_EINVAL on NULL pointers or in_ld < in_len. */
int pss_rebin(const float *in, float *out, int32_t nrows, int64_t in_len, int64_t in_ld,
              int32_t newlen, const int64_t *lo, const int64_t *hi, void *stream);

/* Telescope.observe tail (telescope.py:140-145): clip from above at `clip`,
 * cast to float32 or int8 (truncation toward zero, as numpy's astype). */
int pss_clip_cast(const float *in, void *out, int64_t count, float clip, int32_t out_kind,
                  void *stream);

/* Backend.fold (telescope/backend.py:34-49): out[c][b] =
 * sum_{f<n_fold} data[c][npbins + f*half + b], half = npbins/2. */
int pss_fold(const float *data, float *out, int32_t nchan, int64_t ld, int64_t npbins,
             int64_t n_fold, void *stream);

/* Corrected fold (extension, no reference
 * counterpart -- backend.py:34-49 is only valid for exactly four periods):
 * out[c][b] = sum_{p<nper} data[c][p*nbin + b] over whole periods of `nbin`
 * samples, float64 accumulation, float32 out. */
int pss_fold_periods(const float *data, float *out, int32_t nchan, int64_t ld, int64_t nbin,
                     int64_t nper, void *stream);

/*
 * Native host planning (no GPU; bitwise replicas of the float64 NumPy
 * arithmetic in psrsigsim_amd/pulsar/portraits.py, itself pinned to the
 * reference's scipy PCHIP -- pulsar/portraits.py:200-267 of the reference).
 * `nthreads` host threads split the rows.
 *   pss_host_pchip_coef:   c[rows][K-1][4] piecewise-cubic coefficients
 *                          (powers 3..0 of t - x_i) through y[rows][K] at x[K]
 *   pss_host_ppoly_eval:   out[rows][n] = the cubic at phases ph[n]
 *                          (interval = last x_i <= phase, end pieces extrapolate)
 *   pss_host_device_table: out[rows][nint][4] (float32) = c * (h^3, h^2, h, 1)
 *                          / amax (the table the source stage evaluates)
 *   pss_host_pchip_eval:   pchip_coef then ppoly_eval (then / div when div != 1)
 *                          fused per row: no coefficient table in memory
 *   pss_host_pchip_table:  pchip_coef then device_table fused per row (hcell = h)
 */
int pss_host_pchip_coef(const double *x, int64_t K, const double *y, int64_t rows, double *c,
                        int nthreads);
int pss_host_ppoly_eval(const double *x, int64_t K, const double *c, int64_t rows, const double *ph,
                        int64_t n, double *out, int nthreads);
int pss_host_device_table(const double *c, int64_t rows, int64_t nint, double h, double amax,
                          float *out, int nthreads);
int pss_host_pchip_eval(const double *x, int64_t K, const double *y, int64_t rows, const double *ph, int64_t n,
                        double div, double *out, int nthreads);
int pss_host_pchip_table(const double *x, int64_t K, const double *y, int64_t rows, double hcell, double amax,
                         float *out, int nthreads);

/* Pulsar.null's shift_val (pulsar/pulsar.py:285-288) on the device:
 *   shift_val = count / 2 - argmax(row[0:count])
 * out[0] = shift_val (int64), out[1] = status: 0 ok; 1 the maximum is not
 * unique; 2 a NaN in the row (the reference's np.where then yields 0 or >1
 * indices and the broadcast raises ValueError).  Stream-ordered, no host
 * synchronisation: the fused run reads out[0] through
 * PssPipeline.null_shift_dev. */
int pss_null_shift(const float *row, int64_t count, int64_t *out, void *stream);

/* Philox chi2 draws (test hook + CPU-independent statistics checks):
 * out[r][n] = chi2(df) keyed like the pipeline's purpose `purpose`. */
int pss_chi2_fill(float *out, int32_t nrows, int32_t chan0, int64_t n, float df,
                  uint64_t seed, uint32_t call_id, uint32_t purpose, void *stream);

/*
 * Search-mode output (extension, no reference counterpart).  The input is
 * data[nchan][ld] float32; a file row r holds the nsblk consecutive samples
 * [r*nsblk, (r+1)*nsblk) of every channel, rows counted from the `data`
 * pointer (offset it by whole rows to work in chunks).  One polarisation.
 *
 * pss_chan_stats: mn / mx (float32) and sum / sumsq (float64) [nrows][nchan]
 * of every (row, channel) block.  The float64 sums run in a fixed order
 * (no atomics): the same input gives the same bits, aligned or not.  A NaN in
 * a block makes its four values NaN.
 */
int pss_chan_stats(const float *data, int32_t nchan, int64_t ld, int64_t nsblk, int64_t nrows,
                   float *mn, float *mx, double *sum, double *sumsq, void *stream);

/*
 * pss_quantize_tmajor: out[r][t][c], channel fastest, nchan*nbits/8 bytes per
 * time sample, nbits in {8, 4, 2}:
 *   code = clamp(rint((x - offs[r][c]) / scl[r][c]), 0, 2^nbits - 1)
 * rounding half to even; a NaN x or scl == 0 gives code 0.  For nbits < 8 the
 * lower-numbered channel takes the more significant bits of its byte.
 * nchan*nbits must fill whole bytes.  scl / offs are float32 [nrows][nchan]
 * device arrays.
 */
int pss_quantize_tmajor(const float *data, int32_t nchan, int64_t ld, int64_t nsblk, int64_t nrows,
                        const float *scl, const float *offs, int32_t nbits, void *out, void *stream);

/*
 * Search-mode input (extension, no reference counterpart): the inverse of
 * pss_quantize_tmajor.  in[r][t][p][c] holds nbits-bit codes, nbits in
 * {8, 4, 2}, channel fastest as a SUBINT row's DATA column: every time sample
 * is npol runs of nchan*nbits/8 bytes, the lower-numbered channel in the more
 * significant bits of its byte; nchan*nbits must fill whole bytes.  scl / offs
 * are float32 [nrows][npol][nchan] device arrays (DAT_SCL / DAT_OFFS as
 * stored: a 0 scale is a 0 scale), wts float32 [nrows][nchan] or NULL (all
 * ones).  out is [nchan][ld] float32; row r fills the columns [r*nsblk,
 * (r+1)*nsblk) counted from the `out` pointer (offset out by whole rows of
 * nsblk samples and in / scl / offs / wts by whole rows to work in chunks):
 *   v_p = fmaf((float)code - zero_off, scl[r][p][c], offs[r][p][c])    p < nsum
 *   x   = (nsum == 2 ? v_0 + v_1 : v_0) * w[r][c]
 *   out[flip ? nchan-1-c : c][r*nsblk + t] = x
 * in float32, one rounding per operation on every path.  npol is 1, 2 or 4,
 * nsum 1 or 2 and <= npol; polarisations at or beyond nsum are never read.
 * Whole-dword loads and 16-B stores when the byte runs are a multiple of 4,
 * `in` is 4-B aligned, out and ld are on the 16-B grid and nsblk % 4 == 0;
 * element by element otherwise, the same bits.  No atomics: the same input
 * gives the same bits from run to run.
 * PSS_EINVAL (nothing launched) on NULL in / scl / offs / out, nbits, npol or
 * nsum out of range, channel bits that do not fill whole bytes, nsblk < 1,
 * ld < nrows*nsblk or nchan > 65535; PSS_OK with nothing launched when
 * nchan <= 0 or nrows <= 0.
 */
int pss_unpack_tmajor(const void *in, int32_t nchan, int32_t npol, int32_t nsum, int64_t nsblk, int64_t nrows,
                      const float *scl, const float *offs, const float *wts, float zero_off, int32_t nbits,
                      int32_t flip, float *out, int64_t ld, void *stream);

/*
 * Baseband channeliser and detector (extension, no reference counterpart).
 * x[npol][ld] float32 voltages (npol = 1 or 2, n samples per row), C = nchan a
 * power of two in [16, 4096], L = 2 C, T = ntap in [1, 8], h[T L] the
 * prototype filter (all ones for T = 1):
 *   y_m[j]    = sum_{t<T} h[t L + j] x[(m + t) L + j]            (j < L)
 *   X_m[k]    = sum_j y_m[j] exp(-2 pi i j k / L)
 *   out[k][s] = 1 / (L tscrunch) sum_pol sum_{m = s tscrunch}^{(s+1) tscrunch - 1} |X_m[k]|^2
 * for k < C (bin 0 kept, the Nyquist bin dropped) and s < S = floor(M /
 * tscrunch), M = floor(n / L) - T + 1 spectra; trailing samples and a ragged
 * last group are dropped.  out is [C][out_ld] float32, written once; x is read
 * once.  Sums run in a fixed order: the same input gives the same bits.
 * PSS_EINVAL (nothing launched) on NULL pointers, ld < n, out_ld < S or a
 * parameter out of range; PSS_OK with nothing launched when S < 1.
 */
int pss_channelize(const float *x, int32_t npol, int64_t n, int64_t ld, const float *h, int32_t nchan,
                   int32_t ntap, int32_t tscrunch, float *out, int64_t out_ld, void *stream);

/*
 * Amplitude radiometer noise (receiver.py:123-138): rows[r][i] += scale *
 * N(0, 1) for r < nrows, i < n, in place and stream-ordered.  The draws are
 * the Philox Box-Muller normals of the amplitude pulses, purpose P_NOISE,
 * keyed (seed, call_id, r, i): independent of the launch geometry.
 */
int pss_normal_add(float *rows, int32_t nrows, int64_t n, int64_t ld, float scale, uint64_t seed,
                   uint32_t call_id, void *stream);

/*
 * Incoherent dedispersion over trial DMs (extension, no reference
 * counterpart): the DM-time plane of data[nchan][ld] float32 (n samples per
 * row) for the device table delays[ndm][nchan] of int32 sample delays.  With
 * T = n - max_delay:
 *   d(j, c)   = min(max(delays[j * nchan + c], 0), max_delay)
 *   out[j][t] = sum_{c < nchan} data[c * ld + t + d(j, c)],   t < T, j < ndm
 * the exact direct sum.  The table is arbitrary (it need not be monotone in c
 * or j); because of the clamp no read leaves [0, n) of its row whatever it
 * holds, and nothing is written outside out[j * out_ld + 0 .. T).  A workgroup
 * owns 2048 times of 8 neighbouring trials; a channel whose delays differ by
 * at most 2044 samples among those 8 trials is read from global memory once
 * for all of them (staged in LDS), a channel with a wider spread once per
 * trial.  Every out[j][t] is summed in increasing c by one thread, without
 * atomics: the same input gives the same bits from run to run, and whatever
 * the alignment of data / ld / out / out_ld.  No workspace.
 * PSS_EINVAL (nothing launched) on a NULL pointer, nchan < 1, ndm < 1,
 * ld < n, max_delay < 0, max_delay >= n or out_ld < T, and when
 * ceil(T / 2048) * ceil(ndm / 8) exceeds 2^31 - 1 (the launch grid).
 */
int pss_dedisperse(const float *data, int32_t nchan, int64_t n, int64_t ld, const int32_t *delays,
                   int32_t ndm, int32_t max_delay, float *out, int64_t out_ld, void *stream);

/*
 * Banded dedispersion from several source planes (extension, no reference
 * counterpart): pss_dedisperse's direct sum taken over bands of `band`
 * neighbouring channels, each trial reading the plane of its source -- both
 * stages of the two-stage sub-band dedispersion are calls of it.
 * data holds nsrc planes [nchan][ld] float32 (n samples per row), src_stride
 * floats apart; delays[ndm][nchan] is a device table of int32 sample delays.
 * With nb = ceil(nchan / band) bands (the last may be short), T = n -
 * max_delay and q(j) = min(j / per_src, nsrc - 1) the source of trial j:
 *   d(j, c) = min(max(delays[j * nchan + c], 0), max_delay)
 *   out[(j * nb + s) * out_ld + t]
 *           = sum_{c = s band .. min(nchan, (s + 1) band) - 1}
 *                 data[q(j) * src_stride + c * ld + t + d(j, c)],   t < T, j < ndm, s < nb
 * out is [ndm][nb][out_ld].  Stage 1 of the sub-band scheme is nsrc = 1,
 * per_src >= ndm (every trial reads the one plane); stage 2 is data = stage
 * 1's output, nsrc = its trials, per_src = the trials built from each,
 * nchan = band (one band: out is [ndm][out_ld]).
 * The table is arbitrary; because of the clamp no read leaves [0, n) of its
 * row whatever it holds, and nothing is written outside the T samples of each
 * output row.  pss_dedisperse's tile: a workgroup owns 2048 times of 8
 * neighbouring trials of one source and one band -- the trials are cut into
 * groups of 8 inside each source, so no workgroup reads two sources -- and a
 * channel whose delays differ by at most 2044 samples among them is read once
 * for all (staged in LDS), a wider one once per trial.  Every output is
 * summed in increasing c by one thread, without atomics: the same input gives
 * the same bits from run to run and whatever the alignment of data / ld /
 * src_stride / out / out_ld; with nsrc = 1 and band >= nchan they are
 * pss_dedisperse's bits.  No workspace.
 * PSS_EINVAL (nothing launched) on a NULL pointer, nsrc < 1, nchan < 1,
 * ndm < 1, per_src < 1, band < 1, ld < n, src_stride < nchan * ld,
 * max_delay < 0, max_delay >= n or out_ld < T, and when ceil(T / 2048) * nb *
 * (trial groups) exceeds 2^31 - 1 (the launch grid).
 */
int pss_dedisperse_banded(const float *data, int32_t nsrc, int64_t src_stride, int32_t nchan, int64_t n,
                          int64_t ld, const int32_t *delays, int32_t ndm, int32_t per_src, int32_t max_delay,
                          int32_t band, float *out, int64_t out_ld, void *stream);

/*
 * RFI excision of a search-mode filterbank (extension, no reference
 * counterpart): data[nchan][ld] float32 (n samples per row), mask[nblk][nchan]
 * bytes (non-zero = flagged) over blocks of `block` samples, base[nchan] the
 * channels' replacement value / baseline, rgood[nblk] = float32(1 / number of
 * unflagged channels of the block), 0 where there is none (the kernel never
 * divides; NULL iff zero_dm = 0).  With b(t) = min(t / block, nblk - 1) -- the
 * ragged tail belongs to the last block -- and good(c, t) = !mask[b(t) *
 * nchan + c], all arithmetic IEEE float32, every line one rounded operation:
 *   zero_dm = 0:  out[c][t] = good ? data[c][t] : base[c]
 *   zero_dm = 1:  S[t]      = sum_{c good} (data[c][t] - base[c])
 *                 z[t]      = S[t] * rgood[b(t)]
 *                 out[c][t] = good ? data[c][t] - z[t] : base[c]
 *                 zser[t]   = z[t]                    (when zser != NULL; [n])
 * A flagged sample never enters a sum: a NaN or 1e30 in a flagged cell reaches
 * no output; a NaN in a good cell reaches z[t] and sample t of every good
 * channel only.  Summation order (a pure function of nchan): the channels are
 * split into the 8 contiguous ranges [q P, min((q + 1) P, nchan)), P =
 * ceil(nchan / 8); each range is summed in increasing c into an accumulator
 * that starts at +0 (flagged cells skipped), and the partial sums A_q are
 * combined as ((A_0 + A_1) + (A_2 + A_3)) + ((A_4 + A_5) + (A_6 + A_7)).  The
 * bits depend on neither n, block, the alignment of data / ld / out / out_ld,
 * zser nor the run.  No atomics, no workspace.  out == data with out_ld == ld
 * (in place) is allowed and gives the bits of the out-of-place run; nothing is
 * written outside out[c * out_ld + 0 .. n) and zser[0 .. n).
 * PSS_EINVAL (nothing launched) on a NULL data, mask, base or out, rgood NULL
 * with zero_dm = 1, zero_dm not 0 or 1, nchan < 1, n < 1, ld < n, out_ld < n,
 * block < 1, nblk < 1, (nblk - 1) * block >= n, any other overlap of the
 * extents of out and data, and when ceil(n / 256) exceeds 2^31 - 1 (the
 * launch grid).
 */
int pss_rfi_clean(const float *data, int32_t nchan, int64_t n, int64_t ld, const uint8_t *mask,
                  int64_t block, int64_t nblk, const float *base, const float *rgood, int32_t zero_dm,
                  float *out, int64_t out_ld, float *zser, void *stream);

/*
 * Single-pulse search of a DM-time plane (extension, no reference
 * counterpart): a boxcar matched filter over the widths 2^k, k < nw, of
 * plane[ndm][ld] float32 (T samples per row), normalised per trial by the
 * device arrays mean[ndm] / rstd[ndm] and reduced to one result per cell of
 * `cell` start times, nq = ceil(T / cell) cells per trial.  All arithmetic is
 * IEEE float32, every line one rounded operation:
 *   y[t]       = plane[j * ld + t] - mean[j]                      t < T
 *   S_0[t]     = y[t]
 *   S_{k+1}[t] = S_k[t] + S_k[t + 2^k]                            t + 2^(k+1) <= T
 *   c[j][k]    = a_k * rstd[j],  a_k = 2^-ceil(k/2) * (k odd ? 0x3FB504F3 : 1)
 *   z_k[t]     = S_k[t] * c[j][k]                                 k < nw, t + 2^k <= T
 *   cell q     : the lexicographic maximum of (z, -k, -t) over all (k, t) with
 *                q * cell <= t < min((q + 1) * cell, T) and t + 2^k <= T:
 *                the largest z; ties go to the narrower width, then to the
 *                earlier time; a NaN z never wins
 *   snr[j * out_ld + q]  = that z, -inf if no candidate was greater than -inf
 *   code[j * out_ld + q] = (k << 16) | (t - q * cell), 0 with a -inf result
 * a_k is 2^(-k/2) (0x3FB504F3 is float32(sqrt 2)), so z is the box sum in
 * units of its own standard deviation when rstd = 1 / sigma.  The balanced
 * tree is part of the contract (prefix-sum differences round differently): the
 * bits depend on neither the tile, the alignment of plane / ld / out_ld nor
 * the run.  Widths with 2^k > T do not exist.  A candidate is valid by its
 * index alone: no read leaves [0, T) of its row, and nothing is written
 * outside snr / code [j * out_ld + 0 .. nq).  A workgroup owns 2048 start
 * times of one trial and reads them and 2^(nw-1) - 1 samples of halo (rounded
 * up to 256) once; no atomics, no workspace.
 * PSS_EINVAL (nothing launched) on a NULL pointer, ndm < 1, T < 1, ld < T,
 * nw outside [1, 13], cell not a power of two in [16, 2048], out_ld < nq,
 * and when ceil(T / 2048) * ndm exceeds 2^31 - 1 (the launch grid).
 */
int pss_boxcar_search(const float *plane, int32_t ndm, int64_t T, int64_t ld, const float *mean,
                      const float *rstd, int32_t nw, int32_t cell, float *snr, int32_t *code,
                      int64_t out_ld, void *stream);

/*
 * Periodicity search of a DM-time plane (extension, no reference
 * counterpart): the incoherent harmonic sum of the power spectrum of every
 * trial.  spec[ndm][ld] is a complex spectrum (interleaved float32 re / im, ld
 * in complex elements, nbin usable bins per row -- the rfft of a trial without
 * its Nyquist bin), scale[ndm] a device array; per trial and per cell of `cell`
 * consecutive bins, nq = ceil(nbin / cell) cells, the best sum of 2^l
 * harmonics, l < nl, is kept.  All arithmetic is IEEE float32, every line one
 * rounded operation, no fused multiply-add:
 *   P[k]       = ((re_k * re_k) + (im_k * im_k)) * scale[j]             k < nbin
 *   idx(k,m,h) = floor((k * m + h/2) / h)    (integers, h/2 = 0 at h = 1: the
 *                                             bin nearest to k m / h, <= k)
 *   H_0[k]     = P[k]
 *   H_l[k]     = H_{l-1}[k], then for m = 1, 3, 5 .. h - 1 (h = 2^l) in that
 *                order:  H += P[idx(k,m,h)]
 *   z_l[k]     = (H_l[k] - h) * a_l,  a_l = 2^-ceil(l/2) * (l odd ? 0x3FB504F3 : 1)
 *   valid      : l < nl, k < nbin, idx(k,1,h) >= kmin
 *   cell q     : the lexicographic maximum of (z, -l, -k) over the valid (l, k)
 *                with q * cell <= k < min((q + 1) * cell, nbin): the largest z;
 *                ties go to the lower level, then to the lower bin; a NaN z
 *                never wins
 *   snr[j * out_ld + q]  = that z, -inf if no candidate was greater than -inf
 *   code[j * out_ld + q] = (l << 16) | (k - q * cell), 0 with a -inf result
 * k is the bin of the highest of the h harmonics and the fundamental sits at
 * k / h bins (summing from the top): every term of a sum lies at or below k,
 * and at or above the fundamental's bin, so no read leaves [kmin, nbin) of the
 * row.  The even m of level l are the terms of level l - 1 (idx(k, 2m', 2h') =
 * idx(k, m', h')), which makes the recurrence the full sum over m = 1 .. h.
 * a_l is 2^(-l/2) as in pss_boxcar_search; with scale = 1 / (sigma^2 n) for a
 * series of n samples of variance sigma^2 the powers of white noise are exp(1)
 * variables and z is the sum in units of its own standard deviation.  The
 * fixed order of the adds makes the bits independent of the tile, the
 * alignment of spec / ld / out_ld and the run.  Nothing is written outside
 * snr / code [j * out_ld + 0 .. nq).  A workgroup owns 2048 bins k of one
 * trial and gathers the terms; no atomics.
 * work is NULL or a device buffer of ndm * nbin floats.  With it a first pass
 * writes the powers P[j][k], kmin <= k < nbin, there and the sums gather
 * dwords from rows half as long as the spectrum's, each power computed once
 * rather than once per term -- faster from nl = 4 on, twice as fast at nl = 5,
 * and slower below, down to nl = 1, where every bin is read once anyway
 * (measured: DESIGN.md section 9).
 * Without it the sums gather from the spectrum itself.  The operations and
 * their order are the same either way, and so are the bits; work holds
 * nothing of use afterwards and must not overlap the other buffers.
 * PSS_EINVAL (nothing launched) on a NULL pointer other than work, ndm < 1,
 * nbin < 1, nbin > 2^27 (k * 16 + 8 in 31 bits), ld < nbin, nl outside [1, 5],
 * kmin < 1, cell not a power of two in [16, 2048], out_ld < nq, and when
 * ceil(nbin / 2048) * ndm exceeds 2^31 - 1 (the launch grid).
 */
int pss_harmonic_search(const float *spec, int32_t ndm, int64_t nbin, int64_t ld, const float *scale,
                        int32_t nl, int64_t kmin, int32_t cell, float *snr, int32_t *code, int64_t out_ld,
                        float *work, void *stream);

/*
 * Fold of dedispersed series at fractional periods (extension, no reference
 * counterpart): the phase x time cube of periodicity candidates.  x[nser][ld]
 * float32 holds T samples per row; src[nrows] (int32), inc[nrows] and
 * phi0[nrows] (uint64) are device tables, phi0 may be NULL (all zero).  Output
 * row r folds one series at its own period into nsub sub-integrations of L
 * samples and nbin phase bins.  Phases are 64-bit fixed point, a turn is 2^64,
 * all arithmetic on them wrapping uint64 -- no floating point enters a bin:
 *   inc        = floor(2^64 / Ps + 1/2)        (the caller's; Ps the period in samples)
 *   i(r)       = min(max(src[r], 0), nser - 1)
 *   inc(r)     = min(inc[r], floor(2^64 / nbin))            (Ps >= nbin)
 *   phi_r(u)   = (phi0[r] + u * inc(r)) mod 2^64            u = 0, 1, 2 ..
 *   bin_r(u)   = ((phi_r(u) >> 32) * nbin) >> 32            in [0, nbin), any nbin
 *   out [(r * nsub + s) * nbin + b] = float32(sum of x[i(r) * ld + u] over
 *                                     s L <= u < (s + 1) L with bin_r(u) = b)
 *   hits[(r * nsub + s) * nbin + b] = the number of such u  (int32; hits may be NULL)
 * for r < nrows, s < nsub, b < nbin; both outputs are contiguous
 * [nrows][nsub][nbin], and a bin without a sample holds 0.  Samples at
 * u >= nsub * L are not read.  A sum is accumulated in float64 and rounded to
 * float32 once.  A workgroup owns one (r, s); a bin's samples are added in the
 * order of u by one thread when nbin > 128, and otherwise by G = floor(256 /
 * nbin) threads whose partial sums are then added in the order g = 0 .. G - 1.
 * With n = floor(2^64 / inc(r)): for n <= floor(4096 / G) and for n >= 2^40
 * thread g takes the turns g, g + G, .. of the bin, counted from the
 * sub-integration's first sample (a run of the bin already under way there
 * goes to g = 0); in between it takes the samples g q <= i < (g + 1) q of
 * every run of the bin, i counted from the run's first sample (which may lie
 * before the sub-integration), q = ceil((1 + floor(Wmax / inc(r))) / G), Wmax
 * = ceil(2^32 / nbin) 2^32.  That order is a function of (L, nbin, inc(r),
 * phi_r(s L)) alone, so the bits depend on neither the run, the alignment of
 * x / ld / out, the position of the row in the table nor the other rows of the
 * call.  No atomics, no workspace; nothing is written outside out / hits, and
 * because of the two clamps no read leaves [0, nsub * L) of a row of x
 * whatever the tables hold (inc = 0 is valid: every sample falls in the bin of
 * phi0).
 * PSS_EINVAL (nothing launched) on a NULL x / src / inc / out, nser < 1,
 * nrows < 1, nsub < 1, L < 1, nsub * L > T, ld < T, nbin outside [2, 1024],
 * and when nrows * nsub exceeds 2^31 - 1 (the launch grid).
 */
int pss_fold_series(const float *x, int32_t nser, int64_t T, int64_t ld, const int32_t *src,
                    const uint64_t *inc, const uint64_t *phi0, int32_t nrows, int32_t nsub, int64_t L,
                    int32_t nbin, float *out, int32_t *hits, void *stream);

/*
 * Time-domain resampling of dedispersed series for trial accelerations
 * (extension, no reference counterpart): the first stage of an acceleration
 * search.  x[nser][ld] float32 holds T samples per row; src[nrows] (int32),
 * kappa[nrows] (int64) and sub[nrows] (float32; may be NULL) are device tables.
 * Output row r is series i(r) read at the quadratically stretched times
 * t + alpha t (T - t), alpha = kappa / 2^64 per sample -- integers only, no
 * floating point enters an index:
 *   i(r)     = min(max(src[r], 0), nser - 1)
 *   K(r)     = min(|kappa[r]|, floor(2^63 / T))      (the magnitude taken in
 *                                  uint64), sg(r) = -1 if kappa[r] < 0, else +1
 *   u(t)     = t (T - t)            (T, not n_out: cutting the output short does
 *                                    not change the map)
 *   s_r(t)   = (u(t) K(r) + 2^63) >> 64      the 128-bit product, rounded half up
 *   idx_r(t) = min(max(t + sg(r) s_r(t), 0), T - 1)
 *   out[r * out_ld + t] = x[i(r) * ld + idx_r(t)] - sub[r]      t < n_out, r < nrows
 * The subtraction is one rounded float32 operation; with sub == NULL the bits
 * are copied (a NaN's payload and -0.0 included).  kappa is the caller's
 * alpha 2^64 in fixed point, |alpha| = 4 |s_max| / T^2 for a shift of s_max
 * samples at mid-observation.
 * Bounds.  The clamp of K is alpha T <= 1/2.  With f(t) = u(t) K / 2^64 (a
 * real number), f(t + 1) - f(t) = K (T - 2 t - 1) / 2^64 lies in (-1/2, 1/2),
 * and s = floor(f + 1/2) of two numbers less than 1/2 apart differs by 0, or
 * by 1 in the direction of the difference: s steps by -1, 0 or 1 and idx_r,
 * which adds the step 1 of t, by 0, 1 or 2 -- it is non-decreasing.  u(0) = 0
 * gives idx_r(0) = 0, and f(T - 1) = K (T - 1) / 2^64 < 1/2 gives s = 0 and
 * idx_r(T - 1) = T - 1.  So idx_r runs from 0 to T - 1 without ever leaving
 * [0, T): the index clamp never acts.  It stays in the definition so that no
 * table can make a read leave [0, T) of a row; nothing is written outside
 * out[r * out_ld + 0 .. n_out).  T <= 2^31 - 1 keeps u below 2^62.
 * A workgroup owns 2048 output times of 8 consecutive rows.  The rows among
 * them that read the series of the first and whose source samples fit one
 * window of 4096 floats are served from a copy of that window in LDS, read
 * from global memory once; any other row gathers from global memory.  Every
 * output is one word of x by either route: no atomics, no workspace, and the
 * bits depend on neither the alignment of x / ld / out / out_ld, the position
 * of the row in the table, the other rows of the call nor the run.
 * PSS_EINVAL (nothing launched) on a NULL x / src / kappa / out, nser < 1,
 * nrows < 1, T < 1, T > 2^31 - 1, ld < T, n_out < 1, n_out > T,
 * out_ld < n_out, and when ceil(n_out / 2048) * ceil(nrows / 8) exceeds
 * 2^31 - 1 (the launch grid).
 */
int pss_accel_resample(const float *x, int32_t nser, int64_t T, int64_t ld, const int32_t *src,
                       const int64_t *kappa, const float *sub, int32_t nrows, int64_t n_out, float *out,
                       int64_t out_ld, void *stream);

/*
 * Whitening of a spectrum before pss_harmonic_search (extension, no reference
 * counterpart), two entry points: the lower median of the power over ragged
 * blocks of bins -- the noise spectrum -- and the division of every bin by the
 * median interpolated between block centres, with known interference lines
 * replaced by a neutral value.  spec[ndm][ld] is a complex spectrum
 * (interleaved float32 re / im, ld in complex elements, nbin usable bins per
 * row, as in pss_harmonic_search).  edges[nblk + 1] is a device table of
 * int64, strictly increasing, 0 <= edges[0], edges[nblk] == nbin, every width
 * edges[b + 1] - edges[b] in [1, 256]: block b holds the bins edges[b] ..
 * edges[b + 1] - 1.  The entry points take the device pointer alone and no
 * host copy: the caller validates the table (Backend.whiten_plan builds it on
 * the host).  With a table that breaks these rules the results are not
 * defined, but memory is safe: a block is taken as [e, e + w), e =
 * min(max(edges[b], 0), nbin), w = min(max(edges[b + 1], e), e + 256, nbin) -
 * e, so that no read leaves a row whatever the table holds (w = 0 gives a NaN
 * median), and the whitening reads spec and zap by the bin's own index only.
 * All arithmetic is IEEE float32, every line one rounded operation, no fused
 * multiply-add; division and square root are correctly rounded.
 *
 * pss_spectrum_medians:
 *   P[k]      = (re_k * re_k) + (im_k * im_k)                     k < nbin
 *   key(P)    = 0xFFFFFFFF if P is a NaN, else the bits of P (P >= +0: the
 *               bits order as the values do)
 *   med[j * med_ld + b] = the power whose key stands at sorted index (w - 1) / 2
 *               of the w keys of block b of trial j (the lower median); a NaN
 *               key gives the canonical NaN 0x7FC00000
 * A selection is exact, so the bits depend on neither the algorithm, the tile,
 * the alignment of spec / ld / med_ld nor the run.  Bins below edges[0] enter
 * no block.  Nothing is written outside med[j * med_ld + 0 .. nblk).  A wave
 * owns a block and selects by radix on the 32 key bits (ballots and population
 * counts); a workgroup owns 32 consecutive blocks of one trial.
 *
 * pss_spectrum_whiten, with d_b = edges[b] + edges[b + 1] - 1 (twice the centre
 * of block b, an integer) and m = med + j * med_ld:
 *   norm(k) = m[0]                 if 2 k < d_0 or nblk == 1
 *           = m[nblk - 1]          if 2 k >= d_{nblk-1}
 *           = otherwise, with d_b <= 2 k < d_{b+1}:
 *               f    = float(2 k - d_b) / float(d_{b+1} - d_b)   (both conversions exact)
 *               diff = m[b + 1] - m[b]
 *               t    = diff * f
 *               norm = m[b] + t
 *   q       = LN2 / norm                       LN2 = 0x3F317218
 *   s       = sqrt(q) if 0 < norm < inf, else 0   (a NaN norm: 0)
 *   out[j * out_ld + k] = (re_k * s, im_k * s)                    k < nbin
 * with two rules that take precedence, in this order: a bin k < edges[0] is
 * written as (0, 0); a bin with zap != NULL and zap[k] != 0 is written as
 * (1, 0).  zap is NULL or one uint8[nbin] device table shared by all trials.
 * The median of an exp(1) power of mean mu is mu ln 2: the whitened spectrum of
 * noise has unit mean power and pss_harmonic_search takes it with scale = 1; a
 * zapped bin has exactly the mean power, adds 0 to H - h and can neither make
 * nor spoil a candidate.  out may be spec itself with out_ld == ld (in place)
 * or must not overlap it at all; the bits are the same either way, and depend
 * on neither the tile, the alignment of spec / ld / out / out_ld nor the run.
 * (In place is why there are two entry points: a bin's norm takes the medians
 * of both neighbouring blocks, which a fused kernel would read while another
 * workgroup rewrites them.)  The columns [nbin, out_ld) of a row, the Nyquist
 * bin among them, are never written, and nothing else outside out[j * out_ld +
 * 0 .. nbin).  A workgroup owns 1024 bins of one trial and stages the centres
 * and medians that bracket them in LDS.  No atomics, no workspace beyond med.
 *
 * PSS_EINVAL (nothing launched) on a NULL pointer other than zap, ndm < 1,
 * nbin < 1, nblk < 1, nblk > nbin, ld < nbin, med_ld < nblk, for the whitening
 * out_ld < nbin and an out that overlaps spec without being spec with out_ld
 * == ld, and when ceil(nblk / 32) * ndm (medians) or ceil(nbin / 1024) * ndm
 * (whitening) exceeds 2^31 - 1 (the launch grid).
 */
int pss_spectrum_medians(const float *spec, int32_t ndm, int64_t nbin, int64_t ld, const int64_t *edges,
                         int32_t nblk, float *med, int64_t med_ld, void *stream);
int pss_spectrum_whiten(const float *spec, int32_t ndm, int64_t nbin, int64_t ld, const int64_t *edges,
                        int32_t nblk, const float *med, int64_t med_ld, const uint8_t *zap, float *out,
                        int64_t out_ld, void *stream);

/*
 * Fast folding search of a DM-time plane (extension, no reference
 * counterpart), three entry points: the time scrunch, the folding transform
 * and the search of its profiles.  Common to all three: all arithmetic on data
 * is IEEE float32, every line one rounded operation, no fused multiply-add;
 * all index arithmetic is integer (64-bit wherever a product can pass 2^31);
 * no atomics, no allocation inside the library, no table from the caller.
 *
 * pss_ffa_scrunch: x[nser][ld] float32 holds T samples per row, sub[nser] is a
 * device array or NULL.  The scrunch by 2^lf is a pairwise tree:
 *   y_0[t]        = x[i * ld + t] - sub[i]        (sub == NULL: the bits are copied)
 *   y_{k+1}[u]    = y_k[2u] + y_k[2u + 1]
 *   y[i * y_ld + u] = y_lf[u]                     u < n = T >> lf
 * Samples at and beyond n << lf are not read; nothing is written outside
 * y[i * y_ld + 0 .. n).  Scrunching octave o + 1 from octave o (lf = 1, sub
 * NULL) gives the bits of scrunching from the raw series: the tree is the same.
 * PSS_EINVAL (nothing launched) on a NULL x / y, nser < 1, lf outside [0, 16],
 * T < 1 or T >> lf < 1, ld < T, y_ld < n, and when ceil(n / 256) * nser
 * exceeds 2^31 - 1 (the launch grid).
 */
int pss_ffa_scrunch(const float *x, int32_t nser, int64_t T, int64_t ld, const float *sub, int32_t lf, float *y,
                    int64_t y_ld, void *stream);

/*
 * pss_ffa_transform: y[nser][ld] float32 holds n samples per row.  For series
 * i, base period p = p0 + pi (pi < np) and m = floor(n / p), the leaves are the
 * rows R_r[f] = y[i * ld + r * p + f], r < m, f < p, and the m output profiles
 * F(0, m) come from a top-down halving recursion:
 *   F(a, 1)_0 = R_a
 *   F(a, m), m >= 2:  h = m / 2 (rounded down), t = m - h, H = F(a, h),
 *                     Tl = F(a + h, t); for s < m:
 *     i_s = floor((2 s (h - 1) + (m - 1)) / (2 (m - 1)))
 *     j_s = floor((2 s (t - 1) + (m - 1)) / (2 (m - 1)))
 *     b_s = floor((2 s h       + (m - 1)) / (2 (m - 1)))
 *     F_s[f] = H_{i_s}[f] + Tl_{j_s}[(f + b_s) mod p]           one float32 add
 *   out[((i * np + pi) * n) + s * p + f] = F(0, m)_s[f]
 * Profile s is the fold at the period p + s / (m - 1) samples (m = 1: the
 * series itself).  Words [m p, n) of each block of n are not written and
 * samples [m p, n) of a series are not read.  The tree is part of the
 * contract: the bits depend on neither the tiling, the number of levels a
 * workgroup computes in LDS, the alignment of y / ld / out nor the other
 * periods and series of the call.  Different p of one call can have trees of
 * different depth; a node of one row at an inner level is a copy.  (i_s, j_s,
 * b_s) and a row's node are found by descending the tree per output row, at
 * most 27 uniform integer steps against p adds.
 * work is a second buffer of nser * np * n floats: the levels ping-pong
 * between the two.  It holds nothing of use afterwards and must not overlap
 * out.  The subtree below the first depth whose nodes hold at most 8192
 * floats is computed by one workgroup in LDS in one pass over the block; the
 * levels above it take one pass each.
 * PSS_EINVAL (nothing launched) on a NULL pointer, nser < 1, p0 < 2, np < 1,
 * p0 + np - 1 > min(n, 4096), n > 2^28, ld < n, and when a launch grid
 * (ceil(floor(n / p0) / 4) * nser * np workgroups a level) exceeds 2^31 - 1.
 */
int pss_ffa_transform(const float *y, int32_t nser, int64_t n, int64_t ld, int32_t p0, int32_t np, float *out,
                      float *work, void *stream);

/*
 * pss_ffa_profile_search: a circular boxcar matched filter over the profiles
 * of pss_ffa_transform, taken in its layout (prof = its out, the same nser, n,
 * p0, np), reduced to cells of `cell` consecutive shifts s.  rstd[nser] and
 * rm[np] are device arrays.  With m = floor(n / p) and prof_s the profile s of
 * block (i, pi):
 *   S_0[f]     = prof_s[f]
 *   S_{k+1}[f] = S_k[f] + S_k[(f + 2^k) mod p]
 *   valid (k, f): k < nw, 2^(k+1) <= p, f < p
 *   g          = rstd[i] * rm[pi]                               one rounded product
 *   z_k[f]     = (S_k[f] * a_k) * g       a_k as in pss_boxcar_search
 *   cell q < nq_p = ceil(m / cell): the lexicographic maximum of (z, -k, -s, -f)
 *                over q * cell <= s < min((q + 1) * cell, m): the largest z; ties
 *                go to the narrower width, then to the lower shift, then to the
 *                lower phase; a NaN z never wins
 *   snr  [(i * np + pi) * out_ld + q] = that z, -inf if nothing beat -inf
 *   code [...] = (k << 16) | (s - q * cell)     (0 with -inf)
 *   phase[...] = f                              (0 with -inf)
 *   cells nq_p <= q < nq = ceil(floor(n / p0) / cell) hold -inf, 0, 0
 * Nothing is written at or beyond column nq of a row.  With rm = 1 / sqrt(m)
 * and rstd = 1 / sigma of a sample of the series, z is the box sum in units of
 * its own standard deviation on white noise.
 * PSS_EINVAL (nothing launched) on a NULL pointer, nser < 1, p0 < 2, np < 1,
 * p0 + np - 1 > min(n, 4096), n > 2^28, nw outside [1, 11], cell not a power
 * of two in [16, 2048], out_ld < nq, and when nq * nser * np exceeds 2^31 - 1
 * (the launch grid).
 */
int pss_ffa_profile_search(const float *prof, int32_t nser, int64_t n, int32_t p0, int32_t np, const float *rstd,
                           const float *rm, int32_t nw, int32_t cell, float *snr, int32_t *code, int32_t *phase,
                           int64_t out_ld, void *stream);

/*
 * pss_toa_fit: pulse arrival times from folded profiles (extension, no
 * reference counterpart): Taylor's (1992) Fourier-domain template match
 * (FFTFIT) of every (channel, sub-integration) profile of a fold-mode signal.
 * Profile (c, s), c < nchan, s < nsub, is the N = nbin floats data[c * ld +
 * s * nbin ..): a fold-mode signal's own layout.  It is fitted as p[n] ~ a +
 * b s((n / N) - tau) against the template t = c (ntmpl == nchan) or 0 (ntmpl
 * == 1).  With the unnormalised transforms P_k = sum_n p_n e^{-2 pi i k n / N}
 * and S_k likewise, the harmonics k = 1 .. K, K = min(nharm, (N - 1) / 2) (the
 * Nyquist harmonic is never used), and the template table tspec[ntmpl][K + 1][2]
 * float32 (planned in float64 on the host and rounded once) that holds
 * (Re S_k, Im S_k) at k = 0 .. K (S_0 is needed for the offset a alone):
 *   X_k     = P_k conj(S_k)
 *   C(tau)  = sum_k Re[X_k e^{+2 pi i k tau}]        S2 = sum_k |S_k|^2
 *   coarse  : j* = the first maximum of C on the grid tau_j = j / N, j < N
 *   refine  : the root delta of C' in [-1 / N, 1 / N] around j* / N, by Newton
 *             steps from delta = 0, delta' = delta - g / (2 pi D), g = sum_k k
 *             Im[X_k e^{i phi_k}], D = sum_k k^2 Re[X_k e^{i phi_k}], kept
 *             inside the bracket that the sign of g maintains (g < 0 raises the
 *             lower end; a step of 2^-26 turns or more that leaves the bracket,
 *             or D <= 0, bisects it).
 *             The phase phi_k / 2 pi is ((k j*) mod N) / N, reduced in integers,
 *             plus k delta, brought to [-1/2, 1/2] before the sine.  The
 *             iteration stops at the delta whose step is below 2^-26 turns
 *             (status 0) or after 24 evaluations (status 1).
 *   tau     = j* / N + delta, in turns, wrapped to [-1/2, 1/2): positive when
 *             the profile arrives later than the template
 *   b       = C(tau) / S2                     a = (P_0 - b S_0) / N
 *   R       = sum_k |P_k|^2 - C(tau)^2 / S2
 *   sF2     = max(R, 0) / (2 K - 2), the variance of the real and of the
 *             imaginary part of P_k; K = 1 leaves no degree of freedom: +inf
 *   tau_err = sqrt(sF2 / (b D)) / 2 pi        b_err = sqrt(sF2 / S2)
 *   rms     = sqrt(2 sF2 / N), the noise per bin      snr = b / b_err
 *   out[(c * nsub + s) * out_ld + 0 .. 8) = tau, tau_err, b, b_err, a, rms, snr,
 *             status
 * status 2 is a degenerate fit: C(tau) <= 0 or D <= 0 (a constant profile among
 * them: C = 0) gives tau = the coarse maximum, tau_err = b_err = +inf, snr =
 * b / inf and the other fields by the formulas above; a profile with a
 * non-finite sample gives tau = 0, both errors +inf and NaN in b, a, rms and
 * snr.  A profile's bits depend on its own samples and its template only: not
 * on the profiles beside it, their number, the alignment of data / ld / out /
 * out_ld nor the run.  nbin = 2^m in [32, 4096] takes the FFT path (a profile
 * is one complex sequence of N / 2 points: even and odd bins; a workgroup owns
 * 8192 / nbin profiles and a group of min(64, nbin / 32) lanes refines one);
 * every other nbin the direct path, O(K nbin) per profile with a workgroup
 * each, in float64 sums rounded once.  On either path the sums run over p_n -
 * p_0, which leaves the harmonics k >= 1 as they are and makes a constant
 * profile exact zeros (P_0 gets N p_0 back), and sum |P_k|^2, S2 and C(tau) are
 * float64 sums of float32 terms, R their float64 difference rounded once.  Both read data with 16-B loads where data is on the
 * 16-B grid and ld and nbin are multiples of 4, with element loads otherwise.
 * Nothing is read outside data[c * ld + 0 .. nsub * nbin) and the table,
 * nothing is written outside out[r * out_ld + 0 .. 8).  No atomics, no
 * workspace.
 * PSS_EINVAL (nothing launched) on a NULL pointer, nchan < 1, nsub < 1, nbin
 * outside [8, 8192], ld < nsub * nbin, out_ld < 8, ntmpl other than 1 or
 * nchan, nharm < 1, and when the launch grid (nchan * nsub workgroups on the
 * direct path, an 8192 / nbin-th of it on the FFT path) exceeds 2^31 - 1.
 */
int pss_toa_fit(const float *data, int32_t nchan, int32_t nsub, int32_t nbin, int64_t ld, const float *tspec,
                int32_t ntmpl, int32_t nharm, float *out, int64_t out_ld, void *stream);

/*
 * pss_toa_wide_fit: wideband arrival times (extension, no reference
 * counterpart): one phase and one DM per sub-integration, fitted to all its
 * channels at once (Pennucci, Demorest & Ransom 2014), where pss_toa_fit fits
 * every profile on its own.  data, nchan, nsub, nbin, ld, tspec, ntmpl and
 * nharm are those of pss_toa_fit, and so are N, K, P_k, S_k, X_nk = P_nk
 * conj(S_nk), PP_n = sum_k |P_nk|^2 and S2_n = sum_k |S_nk|^2 of channel n
 * (the same device code forms them, on the same two paths).  Further inputs:
 *   kappa[nchan]  float64: turns of phase per unit of DM, DM_K nu_n^-2 / P
 *   phi0[nchan]   float64: the phase predicted for channel n at the nominal
 *                 DM, reduced to [-1/2, 1/2) on the host
 *   wt[nchan][nsub] float32: 1 / sigma_F^2, the inverse variance of the real
 *                 and of the imaginary part of P_k.  A weight <= 0 or
 *                 non-finite leaves the profile out, and so does a non-finite
 *                 sample in it.  The usable channels of a sub-integration are
 *                 the rest, in index order; every sum over n below runs over
 *                 them alone.
 *   ndm (odd, >= 1), dm_step (>= 0): the coarse grid d_i = i dm_step, |i| <=
 *                 ndm / 2, around the nominal DM (d = 0).
 * For every sub-integration:
 *   phi_n   = phi0_n + phi + kappa_n d
 *   C_n     = sum_k Re[X_nk e^{2 pi i k phi_n}]
 *   F       = sum_n (wt_n / S2_n) C_n^2      (the amplitudes b_n = C_n / S2_n
 *             are profiled out), maximised over (phi, d).
 *   phase   : phi_n is formed and reduced by rint in float64; k phi_n is
 *             formed in float64, reduced by rint and rounded once to float32
 *             for sincospif.  The terms of a harmonic sum are float32
 *             products, their sums float64; everything per channel and above
 *             is float64, the state (phi, d) included.
 *   coarse  : for every d_i, Xbar_k = sum_n wt_n X_nk e^{2 pi i k (phi0_n +
 *             kappa_n d_i)} (channels in index order, float64 sums of float32
 *             terms, rounded once to float32), c_j = sum_k Re[Xbar_k e^{2 pi i
 *             k j / N}], j < N, by float64 sums rounded once to float32 (at
 *             every N), and its first maximum j*(i).  The start is the (d_i,
 *             j* / N wrapped to [-1/2, 1/2)) of the largest value: ties to the
 *             lower |i|, then the lower i, then the lower j.
 *   refine  : with g_n = sum_k k Im[.], D_n = sum_k k^2 Re[.], w_n = wt_n /
 *             S2_n, C'_n = -2 pi g_n, C''_n = -4 pi^2 D_n, q_n = 2 w_n C_n C'_n,
 *             h_n = 2 w_n (C'_n^2 + C_n C''_n): the gradient is (sum q_n, sum
 *             kappa_n q_n), the Hessian H = [[sum h_n, sum kappa_n h_n], [.,
 *             sum kappa_n^2 h_n]], the expected curvature E the same with e_n =
 *             -8 pi^2 w_n C_n^2 T2_n / S2_n, T2_n = sum_k k^2 |S_nk|^2, for
 *             h_n.  The step from a point is p = -H^-1 grad where H is
 *             negative definite (H_11 < 0, det H > 0), else -E^-1 grad, else 0;
 *             it is scaled down so that max(|p_phi|, |p_d| kspan) <= 4 / N (four
 *             bins), kspan = max_n |kappa_n - mean kappa|.  The first
 *             evaluation is at the start.  A trial point x + p is accepted
 *             when |grad(x + p) . p| <= |grad(x) . p|, and a new step is taken
 *             from it; otherwise p is halved.  Values of F are never compared.
 *             When the step to try next has |p_phi| < 2^-26 and |p_d| kspan <
 *             2^-26 turns the fit has converged (status 0): that last step is
 *             taken without an evaluation.  Status 1 after 32 evaluations.
 *   status 2: fewer than two usable channels or kspan = 0 ((phi, d) is the
 *             coarse start, no evaluation), or -H / 2 at the solution not
 *             positive definite: phi_err = d_err = +inf, cov = 0.
 *   out[s * out_ld + 0 .. 10), float64: phi wrapped to [-1/2, 1/2), referred
 *             to infinite frequency; phi_err; d; d_err; cov(phi, d) -- (phi_err^2,
 *             cov; cov, d_err^2) is the inverse of -H / 2 at the solution;
 *             chi2 = sum_n wt_n (PP_n - C_n^2 / S2_n); dof = 2 K n_used - n_used
 *             - 2; n_used; evaluations; status.
 *   prof[(c * nsub + s) * prof_ld + 0 .. 4), float32: b_n, b_err_n = sqrt(1 /
 *             (wt_n S2_n)), the channel's chi2 term, 1 -- or, for a profile
 *             left out, (0, or NaN with a non-finite sample), +inf, 0, 0.
 * A sub-integration's bits depend on its own usable profiles, their entries of
 * the tables and the grid alone: not on nsub, the other sub-integrations, the
 * channels left out (the fit without them gives the same bits), the alignment
 * or strides, nor the run.  Channels are added in blocks of 4 (K > 32), 16 (K >
 * 8) or 64 usable channels, in order, and the blocks in order.  No atomics, no
 * host synchronisation between the launches.  All intermediate storage is
 * work[0 .. pss_toa_wide_workspace_bytes(nchan, nsub, nbin, nharm, ndm)), on
 * the 16-byte grid (0 for arguments pss_toa_wide_fit rejects): X_nk as float2
 * [nsub][nchan][K], the sums of every profile, the channel lists, Xbar_k of
 * every trial, the trials' maxima,
 * the partial sums and the state.
 * PSS_EINVAL (nothing launched) on a NULL pointer, nchan < 1, nsub < 1, nbin
 * outside [8, 8192], ld < nsub * nbin, out_ld < 10, prof_ld < 4, ntmpl other
 * than 1 or nchan, nharm < 1, ndm even or < 1, dm_step negative or non-finite,
 * work_bytes too small, work off the 16-byte grid, and a launch grid above
 * 2^31 - 1.
 */
int64_t pss_toa_wide_workspace_bytes(int32_t nchan, int32_t nsub, int32_t nbin, int32_t nharm, int32_t ndm);
int pss_toa_wide_fit(const float *data, int32_t nchan, int32_t nsub, int32_t nbin, int64_t ld, const float *tspec,
                     int32_t ntmpl, int32_t nharm, const double *kappa, const double *phi0, const float *wt,
                     int32_t ndm, double dm_step, double *out, int64_t out_ld, float *prof, int64_t prof_ld,
                     void *work, int64_t work_bytes, void *stream);
/*
 * pss_toa_wide_stages: the stages first .. last of pss_toa_wide_fit alone, 0
 * <= first <= last <= 3, for timing them (tools/toa_wide_bench.py): 0 the
 * spectra, 1 the channel lists, the coarse trials and the start, 2 the 32
 * rounds of evaluation and step, 3 the final evaluation and the outputs.  The
 * arguments and their checks are those of pss_toa_wide_fit, which is the
 * stages 0 .. 3; a stage reads what the stages before it left in work.
 */
int pss_toa_wide_stages(const float *data, int32_t nchan, int32_t nsub, int32_t nbin, int64_t ld, const float *tspec,
                        int32_t ntmpl, int32_t nharm, const double *kappa, const double *phi0, const float *wt,
                        int32_t ndm, double dm_step, double *out, int64_t out_ld, float *prof, int64_t prof_ld,
                        void *work, int64_t work_bytes, int32_t first, int32_t last, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* PSS_HIP_H */
