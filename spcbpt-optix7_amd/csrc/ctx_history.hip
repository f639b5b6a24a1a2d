// Context: the history reprojection (kernels_reproject.hip) -- capture of the shown image, its reprojection into the current view,
// and the resolve that blends the prior with the film
// (part of the C ABI library: see capi_common.h for the map of its translation units)
#include "capi_common.h"
#include "kernels_denoise.h"
#include "kernels_reproject.h"

using namespace spc;

namespace spc {

// The three passes are links of the film-merge chain like Context::denoise (ctx_features.hip): they see every merge queued before
// them, and no later merge rewrites the film under them.
void Context::free_history() {
    d_hist_rgbn.release(); d_hist_normal_depth.release(); d_prior.release(); d_resolved.release(); d_resolved_frame.release();
    d_hist_var.release(); d_prior_var.release(); d_resolved_var.release();
    have_history = prior_live = have_resolved = false;
    have_hist_var = have_prior_var = have_resolved_var = false;
}

int Context::history_ready(const char* what, bool need_features) {
    if (deferred.active) { error = "a deferred frame is outstanding: spcbpt_merge_deferred(ctx, keep) first"; return SPCBPT_ERR_STATE; }
    if (!d_accum) { error = std::string(what) + " before spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (need_features && !have_features) { error = std::string(what) + " needs the feature buffers: spcbpt_launch_features since the last spcbpt_resize"; return SPCBPT_ERR_STATE; }
    return 0;
}

// The history carries variance exactly while the moments switch is on; a live prior has to bring its own (a history captured while
// the switch was off has none, and what is blended with it then has no variance either).
bool Context::history_variance_now() const { return film_moments && (!prior_live || have_prior_var); }

// the blend of the live prior (if any) with the film, into the resolved planes or -- for a capture -- into H
// With `out_var` (the moments are on) the variance-carrying kernel writes the same blend and its variance beside it.
int Context::resolve_into(uint32_t frames, float* out, uint32_t* frame, float* out_var) {
    ResolveVarParams v;
    memset(&v, 0, sizeof(v));
    ResolveParams& q = v.base;
    q.width = kp.width; q.height = kp.height; q.frames = (float)frames;
    q.prior = prior_live ? d_prior.p : nullptr;
    q.accum = d_accum; q.out = out; q.frame = frame;
    if (!out_var) {
        launch_resolve(q, rstream);
    } else {
        if (!d_m2n) {   // moments on, but no merge since the last resize: every pixel has n = 0 (as in Context::denoise_variance)
            const size_t px = (size_t)kp.width * kp.height;
            HIP_TRY(this, d_m2n.reserve(px * 4));
            HIP_TRY(this, hipMemsetAsync(d_m2n, 0, px * 16, rstream));
        }
        v.prior_var = prior_live ? d_prior_var.p : nullptr;
        v.m2n = d_m2n; v.out_var = out_var;
        launch_resolve_var(v, rstream);
    }
    HIP_TRY(this, hipGetLastError());
    return 0;
}

// spcbpt_history_capture: H = resolve(frames), G = the feature plane, the camera; the span is "history_capture".
int Context::history_capture(uint32_t frames) {
    if (int rc = history_ready("history_capture", true)) return rc;
    if (frames == 0) { error = "history_capture: frames must be >= 1"; return SPCBPT_ERR_INVALID_ARG; }
    next_render_stream();
    if (int rc = chain_wait()) return rc;
    const size_t px = (size_t)kp.width * kp.height;
    if (!d_hist_rgbn) {   // the five planes, at the first capture after a resize or a reset
        HIP_TRY(this, d_hist_rgbn.reserve(px * 4));
        HIP_TRY(this, d_hist_normal_depth.reserve(px * 4));
        HIP_TRY(this, d_prior.reserve(px * 4));
        HIP_TRY(this, d_resolved.reserve(px * 4));
        HIP_TRY(this, d_resolved_frame.reserve(px));
    }
    const bool with_var = history_variance_now();
    if (with_var && !d_hist_var) HIP_TRY(this, d_hist_var.reserve(px * 4));
    time_begin("history_capture", rstream);
    int rc = resolve_into(frames, d_hist_rgbn, nullptr, with_var ? d_hist_var.p : nullptr);
    if (!rc && hipMemcpyAsync(d_hist_normal_depth, d_feat_normal_depth, px * 16, hipMemcpyDeviceToDevice, rstream) != hipSuccess) {
        error = "history_capture: copy of the feature plane failed"; rc = SPCBPT_ERR_HIP;
    }
    time_end();
    if (rc) return rc;
    memcpy(hist_camera.eye, kp.eye, 12); memcpy(hist_camera.U, kp.U, 12); memcpy(hist_camera.V, kp.V, 12); memcpy(hist_camera.W, kp.W, 12);
    hist_width = kp.width; hist_height = kp.height;
    have_history = true;
    have_hist_var = with_var;
    prior_live = have_prior_var = false;
    return chain_end();
}

// spcbpt_history_reproject: the prior of the current view from the history; the span is "reproject".
int Context::history_reproject(const spcbpt_reproject_params& rp) {
    if (int rc = history_ready("history_reproject", true)) return rc;
    if (!have_history || hist_width != kp.width || hist_height != kp.height) { error = "history_reproject needs a captured history of the current film size: spcbpt_history_capture since the last spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (!(rp.sigma_n == rp.sigma_n) || !(rp.sigma_x == rp.sigma_x) || !(rp.max_history == rp.max_history)) { error = "history_reproject: a parameter is not a number"; return SPCBPT_ERR_INVALID_ARG; }
    const float ext[3] = {bbox_hi[0] - bbox_lo[0], bbox_hi[1] - bbox_lo[1], bbox_hi[2] - bbox_lo[2]};
    const float diag = sqrtf(ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2]);
    const float sigma_n = rp.sigma_n > 0.0f ? rp.sigma_n : SPCBPT_REPROJECT_SIGMA_N;
    const float sigma_x = rp.sigma_x > 0.0f ? rp.sigma_x : SPCBPT_REPROJECT_SIGMA_X_FRACTION * (diag > 0.0f ? diag : 1.0f);
    const float max_history = rp.max_history > 0.0f ? rp.max_history : SPCBPT_REPROJECT_MAX_HISTORY;
    next_render_stream();
    if (int rc = chain_wait()) return rc;
    ReprojectParams q;
    memset(&q, 0, sizeof(q));
    memcpy(q.cur.eye, kp.eye, 12); memcpy(q.cur.U, kp.U, 12); memcpy(q.cur.V, kp.V, 12); memcpy(q.cur.W, kp.W, 12);
    q.hist = hist_camera;
    q.step = reproject_step(sigma_n, sigma_x, max_history);
    q.width = kp.width; q.height = kp.height;
    q.normal_depth = d_feat_normal_depth; q.hist_normal_depth = d_hist_normal_depth; q.hist_rgbn = d_hist_rgbn; q.prior = d_prior;
    if (have_hist_var && !d_prior_var) HIP_TRY(this, d_prior_var.reserve((size_t)kp.width * kp.height * 4));
    time_begin("reproject", rstream);
    if (have_hist_var) {   // prior and PV in one pass, the taps' weights computed once
        ReprojectVarParams v;
        memset(&v, 0, sizeof(v));
        v.base = q; v.hist_var = d_hist_var; v.prior_var = d_prior_var;
        launch_reproject_var(v, rstream);
    } else {
        launch_reproject(q, rstream);
    }
    time_end();
    HIP_TRY(this, hipGetLastError());
    prior_live = true;
    have_prior_var = have_hist_var;
    return chain_end();
}

// spcbpt_history_resolve: the shown image -- the prior, where one is live, blended with the film; the span is "resolve".
int Context::history_resolve(uint32_t frames) {
    if (int rc = history_ready("history_resolve", false)) return rc;
    if (frames == 0) { error = "history_resolve: frames must be >= 1"; return SPCBPT_ERR_INVALID_ARG; }
    next_render_stream();
    if (int rc = chain_wait()) return rc;
    const size_t px = (size_t)kp.width * kp.height;
    if (!d_resolved) {   // a resolve before any capture: the film itself, in planes of its own
        HIP_TRY(this, d_resolved.reserve(px * 4));
        HIP_TRY(this, d_resolved_frame.reserve(px));
    }
    const bool with_var = history_variance_now();
    if (with_var && !d_resolved_var) HIP_TRY(this, d_resolved_var.reserve(px * 4));
    time_begin("resolve", rstream);
    const int rc = resolve_into(frames, d_resolved, d_resolved_frame, with_var ? d_resolved_var.p : nullptr);
    time_end();
    if (rc) return rc;
    have_resolved = true;
    have_resolved_var = with_var;
    return chain_end();
}

// spcbpt_history_denoise: Context::denoise_run (ctx_features.hip) from the resolved image and its variance -- k_demodulate_resolved, the
// variance-guided a-trous passes, k_remodulate -- as one "history_denoise" span.  Writes the denoiser's planes only.
int Context::history_denoise(const spcbpt_denoise_params& dp) {
    if (int rc = history_ready("history_denoise", true)) return rc;
    if (!have_resolved) { error = "history_denoise needs a resolved image: spcbpt_history_resolve since the last spcbpt_resize / spcbpt_history_reset"; return SPCBPT_ERR_STATE; }
    if (!have_resolved_var) { error = "history_denoise: the resolved image has no variance -- the moments were off at the capture or resolve (spcbpt_set_film_moments(ctx, 1) before both)"; return SPCBPT_ERR_STATE; }
    if (int rc = denoise_begin("history_denoise", dp)) return rc;
    return denoise_run("history_denoise", dp, SPCBPT_DENOISE_SIGMA_V, d_resolved, true, [&](const DenoiseParams& q) { launch_demodulate_resolved(q, d_resolved_var, rstream); });
}

}  // namespace spc

extern "C" {

int spcbpt_history_capture(spcbpt_ctx* c, uint32_t frames) {
    CTX_CHECK(c);
    return c->history_capture(frames);
}
int spcbpt_history_reproject(spcbpt_ctx* c, const spcbpt_reproject_params* p) {
    CTX_CHECK(c);
    if (!p) { c->error = "null params"; return SPCBPT_ERR_INVALID_ARG; }
    return c->history_reproject(*p);
}
int spcbpt_reproject_params_struct_size(void) { return (int)sizeof(spcbpt_reproject_params); }
int spcbpt_history_resolve(spcbpt_ctx* c, uint32_t frames) {
    CTX_CHECK(c);
    return c->history_resolve(frames);
}
int spcbpt_history_denoise(spcbpt_ctx* c, const spcbpt_denoise_params* p) {
    CTX_CHECK(c);
    if (!p) { c->error = "null params"; return SPCBPT_ERR_INVALID_ARG; }
    return c->history_denoise(*p);
}
int spcbpt_history_reset(spcbpt_ctx* c) {
    CTX_CHECK(c);
    if (c->sync_all()) return SPCBPT_ERR_HIP;   // passes that still read the planes may be queued
    c->free_history();
    return SPCBPT_OK;
}

int spcbpt_read_history(spcbpt_ctx* c, float* resolved_rgba, uint8_t* resolved_rgba8, float* prior_rgba, float* history_rgbn) {
    CTX_CHECK(c);
    if ((resolved_rgba || resolved_rgba8) && !c->have_resolved) { c->error = "read_history: no spcbpt_history_resolve since the last spcbpt_resize / spcbpt_history_reset"; return SPCBPT_ERR_STATE; }
    if (prior_rgba && !c->prior_live) { c->error = "read_history: no prior is live (spcbpt_history_reproject since the last capture)"; return SPCBPT_ERR_STATE; }
    if (history_rgbn && !c->have_history) { c->error = "read_history: no spcbpt_history_capture since the last spcbpt_resize / spcbpt_history_reset"; return SPCBPT_ERR_STATE; }
    if (c->sync_all()) return SPCBPT_ERR_HIP;
    if (int rc = c->check_diag()) return rc;
    const size_t px = (size_t)c->kp.width * c->kp.height;
    if (resolved_rgba) HIP_TRY(c, hipMemcpy(resolved_rgba, c->d_resolved, px * 16, hipMemcpyDeviceToHost));
    if (resolved_rgba8) HIP_TRY(c, hipMemcpy(resolved_rgba8, c->d_resolved_frame, px * 4, hipMemcpyDeviceToHost));
    if (prior_rgba) HIP_TRY(c, hipMemcpy(prior_rgba, c->d_prior, px * 16, hipMemcpyDeviceToHost));
    if (history_rgbn) HIP_TRY(c, hipMemcpy(history_rgbn, c->d_hist_rgbn, px * 16, hipMemcpyDeviceToHost));
    return SPCBPT_OK;
}

int spcbpt_read_history_variance(spcbpt_ctx* c, float* resolved_var, float* prior_var, float* history_var) {
    CTX_CHECK(c);
    const char* off = " (or the moments were off at the capture or resolve: spcbpt_set_film_moments)";
    if (resolved_var && !c->have_resolved_var) { c->error = std::string("read_history_variance: no spcbpt_history_resolve with a variance since the last spcbpt_resize / spcbpt_history_reset") + off; return SPCBPT_ERR_STATE; }
    if (prior_var && !c->have_prior_var) { c->error = std::string("read_history_variance: no prior with a variance is live") + off; return SPCBPT_ERR_STATE; }
    if (history_var && !c->have_hist_var) { c->error = std::string("read_history_variance: no spcbpt_history_capture with a variance since the last spcbpt_resize / spcbpt_history_reset") + off; return SPCBPT_ERR_STATE; }
    if (c->sync_all()) return SPCBPT_ERR_HIP;
    if (int rc = c->check_diag()) return rc;
    const size_t px = (size_t)c->kp.width * c->kp.height;
    if (resolved_var) HIP_TRY(c, hipMemcpy(resolved_var, c->d_resolved_var, px * 16, hipMemcpyDeviceToHost));
    if (prior_var) HIP_TRY(c, hipMemcpy(prior_var, c->d_prior_var, px * 16, hipMemcpyDeviceToHost));
    if (history_var) HIP_TRY(c, hipMemcpy(history_var, c->d_hist_var, px * 16, hipMemcpyDeviceToHost));
    return SPCBPT_OK;
}

}  // extern "C"
