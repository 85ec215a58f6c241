// pss_toa.hip -- pulse arrival times from folded profiles (extension, no
// reference counterpart: the reference hands its folded profiles to an outside
// tool): Taylor's (1992) Fourier-domain template match, FFTFIT, of every
// (channel, sub-integration) profile of a fold-mode signal against a template
// spectrum (include/pss_hip.h has the definitions).  The kernels, k_toa_fft
// and k_toa_direct, live in pss_toa.hpp, which the wideband fit
// (pss_toa_wide.hip) shares; this unit is the entry point of the fit of every
// profile on its own.
#include "pss_toa.hpp"

extern "C" {

int pss_toa_fit(const float *data, int32_t nchan, int32_t nsub, int32_t nbin, int64_t ld, const float *tspec,
                int32_t ntmpl, int32_t nharm, float *out, int64_t out_ld, void *stream) {
    if (!data) return fail(PSS_EINVAL, "toa_fit: data is NULL");
    if (!tspec) return fail(PSS_EINVAL, "toa_fit: tspec is NULL");
    if (!out) return fail(PSS_EINVAL, "toa_fit: out is NULL");
    if (nchan < 1) return fail(PSS_EINVAL, "toa_fit: nchan %d < 1", nchan);
    if (nsub < 1) return fail(PSS_EINVAL, "toa_fit: nsub %d < 1", nsub);
    if (nbin < 8 || nbin > 8192) return fail(PSS_EINVAL, "toa_fit: nbin %d outside [8, 8192]", nbin);
    if (ld < (int64_t)nsub * nbin)
        return fail(PSS_EINVAL, "toa_fit: ld %lld < nsub %d x nbin %d", (long long)ld, nsub, nbin);
    if (out_ld < 8) return fail(PSS_EINVAL, "toa_fit: out_ld %lld < 8", (long long)out_ld);
    if (ntmpl != 1 && ntmpl != nchan) return fail(PSS_EINVAL, "toa_fit: ntmpl %d is neither 1 nor nchan %d", ntmpl, nchan);
    if (nharm < 1) return fail(PSS_EINVAL, "toa_fit: nharm %d < 1", nharm);
    ToaArgs a;
    a.data = data; a.tspec = tspec; a.out = out; a.ld = ld; a.out_ld = out_ld;
    a.nprof = (int64_t)nchan * nsub;
    a.nsub = nsub; a.nbin = nbin;
    a.K = nharm < (nbin - 1) / 2 ? nharm : (nbin - 1) / 2;
    a.per_chan = ntmpl != 1;
    a.wx = nullptr; a.wmeta = nullptr; a.nchan = nchan;
    return launch_toa<false>("toa_fit", a, on_grid16(data, ld) && nbin % 4 == 0, (hipStream_t)stream);
}

}  // extern "C"
