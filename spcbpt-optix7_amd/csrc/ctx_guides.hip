// Context: the reflected-guide pass (kernels_guides.hip) and the switch that makes spcbpt_denoise / spcbpt_denoise_variance read its planes
// (part of the C ABI library: see capi_common.h for the map of its translation units)
#include "capi_common.h"
#include "dev_guides.h"
#include "kernels_guides.h"

using namespace spc;

namespace spc {

void Context::free_guides() {
    d_guide_albedo.release(); d_guide_normal_depth.release();
    have_guides = false;
}

// spcbpt_launch_guides: a link of the film-merge chain like Context::launch_features (ctx_features.hip) -- consecutive launches apply
// their running means in launch order, and a denoise queued behind one sees it.  No other plane is touched, no event counter is
// charged; the kernel-time span is "guides".
int Context::launch_guides(uint32_t subframe, int r0, int r1, int rs, const spcbpt_guide_params& gp) {
    if (deferred.active) { error = "a deferred frame is outstanding: spcbpt_merge_deferred(ctx, keep) first"; return SPCBPT_ERR_STATE; }
    if (!d_accum) { error = "launch_guides before spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (!have_camera) { error = "launch_guides before spcbpt_set_camera"; return SPCBPT_ERR_STATE; }
    if (gp.max_bounces < 0 || gp.max_bounces > 8) { error = "launch_guides: max_bounces must be in 0..8"; return SPCBPT_ERR_INVALID_ARG; }
    if (!(gp.roughness_max == gp.roughness_max) || !(gp.metallic_min == gp.metallic_min)) { error = "launch_guides: a parameter is not a number"; return SPCBPT_ERR_INVALID_ARG; }
    if (rs < 1) rs = 1;
    if (r0 < 0 || (r0 % 8) != 0) { error = "row_begin must be a non-negative multiple of 8 (8-row bands)"; return SPCBPT_ERR_INVALID_ARG; }
    next_render_stream();
    if (int rc = chain_wait()) return rc;
    // the planes: allocated (and zeroed, for the rows a banded launch leaves alone) at the first guide launch after a resize
    const size_t px = (size_t)kp.width * kp.height;
    if (!d_guide_albedo) {
        HIP_TRY(this, d_guide_albedo.reserve(px * 4));
        HIP_TRY(this, d_guide_normal_depth.reserve(px * 4));
        HIP_TRY(this, hipMemsetAsync(d_guide_albedo, 0, px * 16, rstream));
        HIP_TRY(this, hipMemsetAsync(d_guide_normal_depth, 0, px * 16, rstream));
    }
    GuideParams g;
    memset(&g, 0, sizeof(g));
    g.scene = kp.scene;
    memcpy(g.eye, kp.eye, 12); memcpy(g.U, kp.U, 12); memcpy(g.V, kp.V, 12); memcpy(g.W, kp.W, 12);
    g.width = kp.width; g.height = kp.height; g.subframe = subframe;
    g.row_begin = r0; g.row_end = std::min(r1, (int)kp.height); g.row_step = rs;
    g.max_bounces = gp.max_bounces; g.roughness_max = gp.roughness_max; g.metallic_min = gp.metallic_min;
    g.albedo = d_guide_albedo; g.normal_depth = d_guide_normal_depth;
    int rc = ensure_spill((size_t)guide_thread_count(g), true);
    if (rc) return rc;
    g.spill = kp.spill; g.spill_entries = kp.spill_entries; g.diag = kp.diag;
    time_begin("guides", rstream);
    spc::launch_guides(g, rstream);
    time_end();
    HIP_TRY(this, hipGetLastError());
    have_guides = true;
    return chain_end();
}

// The pair of planes spcbpt_denoise / spcbpt_denoise_variance (`who`) hand to Context::denoise_run: null pointers -- the first-hit planes,
// the call's bits as they were -- with the switch at its default, the guide planes with SPCBPT_GUIDES_REFLECTED.
int Context::denoise_planes(const char* who, const float*& albedo, const float*& normal_depth) {
    albedo = normal_depth = nullptr;
    if (denoise_guides != SPCBPT_GUIDES_REFLECTED) return 0;
    if (!have_guides) { error = std::string(who) + " with reflected guides needs the guide planes: spcbpt_launch_guides since the last spcbpt_resize"; return SPCBPT_ERR_STATE; }
    albedo = d_guide_albedo; normal_depth = d_guide_normal_depth;
    return 0;
}

}  // namespace spc

extern "C" {

int spcbpt_launch_guides(spcbpt_ctx* c, uint32_t subframe, int r0, int r1, int rs, const spcbpt_guide_params* p) {
    CTX_CHECK(c);
    if (!p) { c->error = "null params"; return SPCBPT_ERR_INVALID_ARG; }
    return c->launch_guides(subframe, r0, r1, rs, *p);
}
int spcbpt_guide_params_struct_size(void) { return (int)sizeof(spcbpt_guide_params); }

int spcbpt_read_guides(spcbpt_ctx* c, float* albedo_rgba, float* normal_depth_rgba) {
    CTX_CHECK(c);
    if (!c->have_guides) { c->error = "read_guides: no guide launch since the last spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (c->sync_all()) return SPCBPT_ERR_HIP;
    if (int rc = c->check_diag()) return rc;
    const size_t bytes = (size_t)c->kp.width * c->kp.height * 16;
    if (albedo_rgba) HIP_TRY(c, hipMemcpy(albedo_rgba, c->d_guide_albedo, bytes, hipMemcpyDeviceToHost));
    if (normal_depth_rgba) HIP_TRY(c, hipMemcpy(normal_depth_rgba, c->d_guide_normal_depth, bytes, hipMemcpyDeviceToHost));
    return SPCBPT_OK;
}

int spcbpt_set_denoise_guides(spcbpt_ctx* c, int which) {
    CTX_CHECK(c);
    if (which != SPCBPT_GUIDES_FIRST_HIT && which != SPCBPT_GUIDES_REFLECTED) { c->error = "set_denoise_guides: SPCBPT_GUIDES_FIRST_HIT (0) or SPCBPT_GUIDES_REFLECTED (1)"; return SPCBPT_ERR_INVALID_ARG; }
    c->denoise_guides = which;
    return SPCBPT_OK;
}

}  // extern "C"
