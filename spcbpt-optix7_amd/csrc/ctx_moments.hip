// Context: the film's second moment (kernels_moments.hip), the film error and the variance-guided denoiser built on it
// (part of the C ABI library: see capi_common.h for the map of its translation units)
#include "capi_common.h"
#include "kernels_denoise.h"
#include "kernels_moments.h"

using namespace spc;

namespace spc {

void Context::free_moments() {
    d_m2n.release(); d_err_scratch.release();
}

int Context::set_film_moments(bool on) {
    if (on == film_moments) return 0;
    if (!on && adaptive.active) { error = "set_film_moments: adaptive sampling is active and keeps its per-pixel sample counts in the moments plane: spcbpt_adaptive_end first"; return SPCBPT_ERR_STATE; }
    if (!on) {   // the plane goes with the switch: merges that still read it may be queued
        if (sync_all()) return SPCBPT_ERR_HIP;
        free_moments();
        have_hist_var = have_prior_var = have_resolved_var = false;   // the history's variance goes with the switch (its planes stay until the history's go)
    }
    film_moments = on;
    return 0;
}

// finish_frame, after chain_wait and in front of launch_film_merge on the same stream: the second moment of the pixels this launch's
// merge rewrites, from the mean it is about to replace.  The plane is allocated (and zeroed, for the rows a banded launch leaves
// alone) at the first merge after a resize.  The kernel-time span is "moments".
int Context::moments_step() {
    const size_t px = (size_t)kp.width * kp.height;
    if (!d_m2n) {
        HIP_TRY(this, d_m2n.reserve(px * 4));
        HIP_TRY(this, hipMemsetAsync(d_m2n, 0, px * 16, rstream));
    }
    MomentsParams mp;
    memset(&mp, 0, sizeof(mp));
    mp.width = kp.width; mp.height = kp.height; mp.subframe = kp.subframe;
    mp.row_begin = kp.row_begin; mp.row_end = kp.row_end; mp.row_step = kp.row_step;
    mp.accum = d_accum; mp.result = kp.result; mp.m2n = d_m2n;
    time_begin("moments", rstream);
    launch_film_moments(mp, rstream);
    time_end();
    HIP_TRY(this, hipGetLastError());
    return 0;
}

// spcbpt_film_error: two launches behind the last merge queued, on that merge's stream (no link of the chain: the call waits for its
// own result before it returns), and a read-back of 24 bytes.  The kernel-time span is "film_error".
int Context::film_error(spcbpt_film_error_stats* out) {
    if (!film_moments) { error = "film_error needs the film's moments: spcbpt_set_film_moments(ctx, 1) before the frames are rendered"; return SPCBPT_ERR_STATE; }
    if (!d_accum) { error = "film_error before spcbpt_resize"; return SPCBPT_ERR_STATE; }
    out->pixels = 0; out->mean = 0.0; out->max = 0.0;
    if (!d_m2n) return 0;   // no merge since the last resize: no pixel has two samples
    const size_t px = (size_t)kp.width * kp.height;
    const size_t partial_bytes = sizeof(FilmErrorPartial) * (size_t)kFilmErrorMaxBlocks;
    HIP_TRY(this, d_err_scratch.reserve(partial_bytes + sizeof(spcbpt_film_error_stats)));
    hipStream_t s = last_merge_k >= 0 ? rstreams[last_merge_k] : rstream;
    time_begin("film_error", s);
    launch_film_error(d_accum, d_m2n, px, reinterpret_cast<FilmErrorPartial*>(d_err_scratch.p), d_err_scratch.p + partial_bytes, s);
    time_end();
    HIP_TRY(this, hipGetLastError());
    HIP_TRY(this, hipMemcpyAsync(out, d_err_scratch.p + partial_bytes, sizeof(spcbpt_film_error_stats), hipMemcpyDeviceToHost, s));
    HIP_TRY(this, hipStreamSynchronize(s));
    return check_diag();
}

// spcbpt_denoise_variance: Context::denoise_run (ctx_features.hip) from k_demodulate_var's start values -- the film and its moments --
// through the variance-guided a-trous passes, as one "denoise_variance" span.  A link of the film-merge chain like Context::denoise.
int Context::denoise_variance(const spcbpt_denoise_params& dp) {
    if (deferred.active) { error = "a deferred frame is outstanding: spcbpt_merge_deferred(ctx, keep) first"; return SPCBPT_ERR_STATE; }
    if (!d_accum) { error = "denoise_variance before spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (!film_moments) { error = "denoise_variance needs the film's moments: spcbpt_set_film_moments(ctx, 1) before the frames are rendered"; return SPCBPT_ERR_STATE; }
    if (!have_features) { error = "denoise_variance needs the feature buffers: spcbpt_launch_features since the last spcbpt_resize"; return SPCBPT_ERR_STATE; }
    const float *albedo, *normal_depth;
    if (int rc = denoise_planes("denoise_variance", albedo, normal_depth)) return rc;
    if (int rc = denoise_begin("denoise_variance", dp)) return rc;
    if (!d_m2n) {   // moments on, but no merge since the last resize: every pixel has n = 0
        const size_t px = (size_t)kp.width * kp.height;
        HIP_TRY(this, d_m2n.reserve(px * 4));
        HIP_TRY(this, hipMemsetAsync(d_m2n, 0, px * 16, rstream));
    }
    return denoise_run("denoise_variance", dp, SPCBPT_DENOISE_SIGMA_V, d_accum, true, [&](const DenoiseParams& q) { launch_demodulate_var(q, d_m2n, rstream); }, albedo, normal_depth);
}

}  // namespace spc

extern "C" {

int spcbpt_set_film_moments(spcbpt_ctx* c, int enabled) {
    CTX_CHECK(c);
    return c->set_film_moments(enabled != 0);
}
int spcbpt_get_film_moments(spcbpt_ctx* c, int* enabled) {
    CTX_CHECK(c);
    if (!enabled) { c->error = "null pointer"; return SPCBPT_ERR_INVALID_ARG; }
    *enabled = c->film_moments ? 1 : 0;
    return SPCBPT_OK;
}

int spcbpt_read_film_moments(spcbpt_ctx* c, float* m2n_out) {
    CTX_CHECK(c);
    if (!c->film_moments) { c->error = "read_film_moments: the film's moments are off (spcbpt_set_film_moments)"; return SPCBPT_ERR_STATE; }
    if (!c->d_accum) { c->error = "read_film_moments before spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (!m2n_out) { c->error = "null pointer"; return SPCBPT_ERR_INVALID_ARG; }
    if (c->sync_all()) return SPCBPT_ERR_HIP;
    if (int rc = c->check_diag()) return rc;
    const size_t bytes = (size_t)c->kp.width * c->kp.height * 16;
    if (!c->d_m2n) { memset(m2n_out, 0, bytes); return SPCBPT_OK; }   // no merge since the last resize
    HIP_TRY(c, hipMemcpy(m2n_out, c->d_m2n, bytes, hipMemcpyDeviceToHost));
    return SPCBPT_OK;
}

int spcbpt_film_error(spcbpt_ctx* c, spcbpt_film_error_stats* out) {
    CTX_CHECK(c);
    if (!out) { c->error = "null pointer"; return SPCBPT_ERR_INVALID_ARG; }
    return c->film_error(out);
}
int spcbpt_film_error_struct_size(void) { return (int)sizeof(spcbpt_film_error_stats); }

int spcbpt_denoise_variance(spcbpt_ctx* c, const spcbpt_denoise_params* p) {
    CTX_CHECK(c);
    if (!p) { c->error = "null params"; return SPCBPT_ERR_INVALID_ARG; }
    return c->denoise_variance(*p);
}

}  // extern "C"
