// Context: the first-hit feature pass (kernels_features.hip) and the a-trous denoiser that reads it (kernels_denoise.hip)
// (part of the C ABI library: see capi_common.h for the map of its translation units)
#include "capi_common.h"
#include "dev_features.h"
#include "kernels_denoise.h"
#include "kernels_features.h"

using namespace spc;

namespace spc {

// Both passes are links of the film-merge chain (ctx_render.hip: chain_wait / chain_end): they take the next render stream, wait for the
// last link queued and leave ev_merge behind for the next one.  So the running means of consecutive feature launches are applied in
// launch order, a denoise sees every merge queued before it, and no later merge rewrites the film under it -- the order a "pt"
// launch's merge has.
void Context::free_features() {
    d_feat_albedo.release(); d_feat_normal_depth.release();
    d_dn_position.release(); d_dn_ping.release(); d_dn_pong.release(); d_denoised.release(); d_denoised_frame.release();
    have_features = have_denoised = false;
}

// spcbpt_launch_features: the film is not touched, no event counter is charged; the kernel-time span is "features".
int Context::launch_features(uint32_t subframe, int r0, int r1, int rs) {
    if (deferred.active) { error = "a deferred frame is outstanding: spcbpt_merge_deferred(ctx, keep) first"; return SPCBPT_ERR_STATE; }
    if (!d_accum) { error = "launch_features before spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (!have_camera) { error = "launch_features before spcbpt_set_camera"; return SPCBPT_ERR_STATE; }
    if (rs < 1) rs = 1;
    if (r0 < 0 || (r0 % 8) != 0) { error = "row_begin must be a non-negative multiple of 8 (8-row bands)"; return SPCBPT_ERR_INVALID_ARG; }
    next_render_stream();
    if (int rc = chain_wait()) return rc;
    // the buffers: allocated (and zeroed, for the rows a banded launch leaves alone) at the first feature launch after a resize, so
    // that a context that never asks for features keeps its footprint (spcbpt_resize has freed those of the old size)
    const size_t px = (size_t)kp.width * kp.height;
    if (!d_feat_albedo) {
        HIP_TRY(this, d_feat_albedo.reserve(px * 4));
        HIP_TRY(this, d_feat_normal_depth.reserve(px * 4));
        HIP_TRY(this, hipMemsetAsync(d_feat_albedo, 0, px * 16, rstream));
        HIP_TRY(this, hipMemsetAsync(d_feat_normal_depth, 0, px * 16, rstream));
    }
    FeatureParams fp;
    memset(&fp, 0, sizeof(fp));
    fp.scene = kp.scene;
    memcpy(fp.eye, kp.eye, 12); memcpy(fp.U, kp.U, 12); memcpy(fp.V, kp.V, 12); memcpy(fp.W, kp.W, 12);
    fp.width = kp.width; fp.height = kp.height; fp.subframe = subframe;
    fp.row_begin = r0; fp.row_end = std::min(r1, (int)kp.height); fp.row_step = rs;
    fp.albedo = d_feat_albedo; fp.normal_depth = d_feat_normal_depth;
    int rc = ensure_spill((size_t)feature_thread_count(fp), true);
    if (rc) return rc;
    fp.spill = kp.spill; fp.spill_entries = kp.spill_entries; fp.diag = kp.diag;
    time_begin("features", rstream);
    spc::launch_features(fp, rstream);
    time_end();
    HIP_TRY(this, hipGetLastError());
    have_features = true;
    return chain_end();
}

// What the three denoisers share.  denoise_begin: the refusals of `iterations` and of a NaN sigma under the caller's name `who`, then the
// link begins -- what the caller queues on `rstream` from here on (denoise_variance: its zero moments) runs in front of the filter.
int Context::denoise_begin(const char* who, const spcbpt_denoise_params& dp) {
    if (dp.iterations < 1 || dp.iterations > kDenoiseMaxIterations) { error = std::string(who) + ": iterations must be in 1..8"; return SPCBPT_ERR_INVALID_ARG; }
    if (!(dp.sigma_c == dp.sigma_c) || !(dp.sigma_n == dp.sigma_n) || !(dp.sigma_x == dp.sigma_x)) { error = std::string(who) + ": a sigma is not a number"; return SPCBPT_ERR_INVALID_ARG; }
    next_render_stream();
    return chain_wait();
}

// denoise_run: the sigmas (<= 0: the defaults, the colour / variance one the caller's), the five planes at the first call after a resize,
// and the launches as one span `who`: the caller's demodulate of `input` -> `iterations` a-trous passes between the two planes, plain
// or variance-guided -> remodulate + tone map.  Ends the link.
int Context::denoise_run(const char* who, const spcbpt_denoise_params& dp, float sigma_c_default, const float* input, bool variance_guided,
                         const std::function<void(const DenoiseParams&)>& demodulate, const float* albedo, const float* normal_depth) {
    const float ext[3] = {bbox_hi[0] - bbox_lo[0], bbox_hi[1] - bbox_lo[1], bbox_hi[2] - bbox_lo[2]};
    const float diag = sqrtf(ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2]);
    const float sigma_c = dp.sigma_c > 0.0f ? dp.sigma_c : sigma_c_default;
    const float sigma_n = dp.sigma_n > 0.0f ? dp.sigma_n : SPCBPT_DENOISE_SIGMA_N;
    const float sigma_x = dp.sigma_x > 0.0f ? dp.sigma_x : SPCBPT_DENOISE_SIGMA_X_FRACTION * (diag > 0.0f ? diag : 1.0f);
    const size_t px = (size_t)kp.width * kp.height;
    if (!d_denoised) {
        HIP_TRY(this, d_dn_position.reserve(px * 4));
        HIP_TRY(this, d_dn_ping.reserve(px * 4));
        HIP_TRY(this, d_dn_pong.reserve(px * 4));
        HIP_TRY(this, d_denoised_frame.reserve(px));
        HIP_TRY(this, d_denoised.reserve(px * 4));
    }
    DenoiseParams q;
    memset(&q, 0, sizeof(q));
    memcpy(q.U, kp.U, 12); memcpy(q.V, kp.V, 12); memcpy(q.W, kp.W, 12);
    q.width = kp.width; q.height = kp.height;
    q.accum = input; q.albedo = albedo ? albedo : d_feat_albedo.p; q.normal_depth = normal_depth ? normal_depth : d_feat_normal_depth.p;   // (the caller's pair: Context::denoise_planes)
    q.position = d_dn_position; q.ping = d_dn_ping; q.pong = d_dn_pong; q.denoised = d_denoised; q.frame = d_denoised_frame;
    time_begin(who, rstream);
    demodulate(q);
    for (int i = 0; i < dp.iterations; i++) {
        if (variance_guided) launch_atrous_var(q, atrous_var_step(i, sigma_c, sigma_n, sigma_x), (i & 1) == 0, rstream);
        else launch_atrous(q, atrous_step(i, sigma_c, sigma_n, sigma_x), (i & 1) == 0, rstream);
    }
    launch_remodulate(q, (dp.iterations & 1) != 0, rstream);
    time_end();
    HIP_TRY(this, hipGetLastError());
    have_denoised = true;
    return chain_end();
}

// spcbpt_denoise: the plain filter on the film, as one "denoise" span.
int Context::denoise(const spcbpt_denoise_params& dp) {
    if (deferred.active) { error = "a deferred frame is outstanding: spcbpt_merge_deferred(ctx, keep) first"; return SPCBPT_ERR_STATE; }
    if (!d_accum) { error = "denoise before spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (!have_features) { error = "denoise needs the feature buffers: spcbpt_launch_features since the last spcbpt_resize"; return SPCBPT_ERR_STATE; }
    const float *albedo, *normal_depth;
    if (int rc = denoise_planes("denoise", albedo, normal_depth)) return rc;
    if (int rc = denoise_begin("denoise", dp)) return rc;
    return denoise_run("denoise", dp, SPCBPT_DENOISE_SIGMA_C, d_accum, false, [&](const DenoiseParams& q) { launch_demodulate(q, rstream); }, albedo, normal_depth);
}

}  // namespace spc

extern "C" {

int spcbpt_launch_features(spcbpt_ctx* c, uint32_t subframe, int r0, int r1, int rs) {
    CTX_CHECK(c);
    return c->launch_features(subframe, r0, r1, rs);
}

int spcbpt_read_features(spcbpt_ctx* c, float* albedo_rgba, float* normal_depth_rgba) {
    CTX_CHECK(c);
    if (!c->have_features) { c->error = "read_features: no feature launch since the last spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (c->sync_all()) return SPCBPT_ERR_HIP;
    if (int rc = c->check_diag()) return rc;
    const size_t bytes = (size_t)c->kp.width * c->kp.height * 16;
    if (albedo_rgba) HIP_TRY(c, hipMemcpy(albedo_rgba, c->d_feat_albedo, bytes, hipMemcpyDeviceToHost));
    if (normal_depth_rgba) HIP_TRY(c, hipMemcpy(normal_depth_rgba, c->d_feat_normal_depth, bytes, hipMemcpyDeviceToHost));
    return SPCBPT_OK;
}

int spcbpt_denoise(spcbpt_ctx* c, const spcbpt_denoise_params* p) {
    CTX_CHECK(c);
    if (!p) { c->error = "null params"; return SPCBPT_ERR_INVALID_ARG; }
    return c->denoise(*p);
}
int spcbpt_denoise_params_struct_size(void) { return (int)sizeof(spcbpt_denoise_params); }

int spcbpt_read_denoised(spcbpt_ctx* c, float* rgba, uint8_t* rgba8) {
    CTX_CHECK(c);
    if (!c->have_denoised) { c->error = "read_denoised: no spcbpt_denoise since the last spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (c->sync_all()) return SPCBPT_ERR_HIP;
    if (int rc = c->check_diag()) return rc;
    const size_t px = (size_t)c->kp.width * c->kp.height;
    if (rgba) HIP_TRY(c, hipMemcpy(rgba, c->d_denoised, px * 16, hipMemcpyDeviceToHost));
    if (rgba8) HIP_TRY(c, hipMemcpy(rgba8, c->d_denoised_frame, px * 4, hipMemcpyDeviceToHost));
    return SPCBPT_OK;
}

}  // extern "C"
