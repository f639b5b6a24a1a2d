// Context: the local tone stage (kernels_local_tone.hip) -- a base / detail decomposition of log-luminance through a bilateral grid, of
// one of the context's linear images, of the bloom plane or of an image of the caller's, into a float4 plane of its own that
// spcbpt_display can tone-map (SPCBPT_DISPLAY_LOCAL)
// (part of the C ABI library: see capi_common.h for the map of its translation units)
#include "capi_common.h"
#include "kernels_local_tone.h"

using namespace spc;

namespace spc {

void Context::free_local_tone() {
    d_local.release(); d_local_grid[0].release(); d_local_grid[1].release(); d_local_src.release();
    local_last = LocalTone();
}

static const char* local_tone_check(const spcbpt_local_tone_params& p) { return local_tone_params_error(p.cell, p.range, p.blur, p.compress, p.detail, p.anchor); }

// The launches of one call, on `rstream` between chain_wait and chain_end, one span "local_tone": the gather into grid buffer 0, a launch
// per blur pass that goes from one buffer to the other, the slice from the buffer the last pass wrote.
int Context::local_tone_run(const float* src, int width, int height, const spcbpt_local_tone_params& p) {
    const LtPlan plan = local_tone_plan_of(width, height, p.cell, p.range, p.anchor);   // (its node count was checked before the link began)
    const size_t px = (size_t)width * height;
    HIP_TRY(this, d_local.reserve(px * 4));
    HIP_TRY(this, d_local_grid[0].reserve((size_t)plan.nodes * 2));
    HIP_TRY(this, d_local_grid[1].reserve((size_t)plan.nodes * 2));
    LocalToneParams q;
    memset(&q, 0, sizeof(q));
    q.src = src; q.out = d_local; q.grid[0] = d_local_grid[0]; q.grid[1] = d_local_grid[1];
    q.width = width; q.height = height; q.cell = plan.cell; q.gx = plan.gx; q.gy = plan.gy; q.nz = plan.nz;
    q.range = p.range; q.compress = p.compress; q.detail = p.detail; q.la = plan.la;
    time_begin("local_tone", rstream);
    int at = 0;
    launch_local_tone_build(q, at, rstream);
    for (int k = 0; k < p.blur; k++) { launch_local_tone_blur(q, at, rstream); at = 1 - at; }
    launch_local_tone_slice(q, at, rstream);
    time_end();
    HIP_TRY(this, hipGetLastError());
    local_last.have = true; local_last.width = width; local_last.height = height;
    return 0;
}

// spcbpt_local_tone: a link of the film-merge chain like Context::bloom -- it sees every merge, denoise, resolve and bloom queued before
// it, and nothing queued later rewrites its source under it.  Writes its own plane and grid buffers only.  The refusals are
// spcbpt_display's.
int Context::local_tone(int source, const spcbpt_local_tone_params& p) {
    if (const char* bad = local_tone_check(p)) { error = bad; return SPCBPT_ERR_INVALID_ARG; }
    if (source < SPCBPT_DISPLAY_FILM || source > SPCBPT_DISPLAY_BLOOM) { error = "local_tone: source must be 0 (film), 1 (denoised), 2 (robust), 3 (history) or 4 (bloom)"; return SPCBPT_ERR_INVALID_ARG; }
    if (deferred.active) { error = "local_tone: a deferred frame is outstanding: spcbpt_merge_deferred(ctx, keep) first"; return SPCBPT_ERR_STATE; }
    const float* src = nullptr;
    int width = (int)kp.width, height = (int)kp.height;
    if (source == SPCBPT_DISPLAY_BLOOM) {   // the bloom plane, at the size of the image it was made from (spcbpt_bloom_image needs no film)
        if (!bloom_last.have) { error = "local_tone: no bloom plane: spcbpt_bloom / spcbpt_bloom_image since the last spcbpt_resize"; return SPCBPT_ERR_STATE; }
        src = d_bloom; width = bloom_last.width; height = bloom_last.height;
    } else {
        if (!d_accum) { error = "local_tone before spcbpt_resize"; return SPCBPT_ERR_STATE; }
        src = d_accum;
        if (source == SPCBPT_DISPLAY_DENOISED) {
            if (!have_denoised) { error = "local_tone: no denoised image: spcbpt_denoise / spcbpt_denoise_variance / spcbpt_history_denoise since the last spcbpt_resize"; return SPCBPT_ERR_STATE; }
            src = d_denoised;
        } else if (source == SPCBPT_DISPLAY_ROBUST) {
            if (!film_buckets) { error = "local_tone: no robust image: the film's buckets are off (spcbpt_set_film_buckets, then spcbpt_robust_resolve)"; return SPCBPT_ERR_STATE; }
            if (!have_robust) { error = "local_tone: no robust image: no spcbpt_robust_resolve since the film's buckets were last set up"; return SPCBPT_ERR_STATE; }
            src = d_robust;
        } else if (source == SPCBPT_DISPLAY_HISTORY) {
            if (!have_resolved) { error = "local_tone: no resolved history image: spcbpt_history_resolve since the last spcbpt_resize / spcbpt_history_reset"; return SPCBPT_ERR_STATE; }
            src = d_resolved;
        }
    }
    if (local_tone_plan_of(width, height, p.cell, p.range, p.anchor).nodes > kLtMaxNodes) { error = "local_tone: the grid would have more than 2^25 nodes: a larger cell or range"; return SPCBPT_ERR_INVALID_ARG; }
    next_render_stream();
    if (int rc = chain_wait()) return rc;
    if (int rc = local_tone_run(src, width, height, p)) return rc;
    return chain_end();
}

// spcbpt_local_tone_image: the same link over a scratch copy of the caller's image, uploaded behind the chain and waited for, so that
// the caller's image may go when the call returns (Context::bloom_image's way).
int Context::local_tone_image(const float* rgba, int width, int height, const spcbpt_local_tone_params& p) {
    if (const char* bad = local_tone_check(p)) { error = bad; return SPCBPT_ERR_INVALID_ARG; }
    if (!rgba) { error = "null pointer"; return SPCBPT_ERR_INVALID_ARG; }
    if (width < 1 || height < 1 || (int64_t)width * height > (1ll << 28)) { error = "local_tone_image: the image must hold 1 .. 2^28 pixels"; return SPCBPT_ERR_INVALID_ARG; }
    if (local_tone_plan_of(width, height, p.cell, p.range, p.anchor).nodes > kLtMaxNodes) { error = "local_tone: the grid would have more than 2^25 nodes: a larger cell or range"; return SPCBPT_ERR_INVALID_ARG; }
    const size_t px = (size_t)width * height;
    next_render_stream();
    if (int rc = chain_wait()) return rc;
    HIP_TRY(this, d_local_src.reserve(px * 4));
    HIP_TRY(this, hipMemcpyAsync(d_local_src, rgba, px * 16, hipMemcpyHostToDevice, rstream));
    HIP_TRY(this, hipStreamSynchronize(rstream));
    if (int rc = local_tone_run(d_local_src, width, height, p)) return rc;
    return chain_end();
}

}  // namespace spc

extern "C" {

int spcbpt_local_tone(spcbpt_ctx* c, int source, const spcbpt_local_tone_params* p) {
    CTX_CHECK(c);
    if (!p) { c->error = "null params"; return SPCBPT_ERR_INVALID_ARG; }
    return c->local_tone(source, *p);
}

int spcbpt_local_tone_image(spcbpt_ctx* c, const float* rgba, int width, int height, const spcbpt_local_tone_params* p) {
    CTX_CHECK(c);
    if (!p) { c->error = "null params"; return SPCBPT_ERR_INVALID_ARG; }
    return c->local_tone_image(rgba, width, height, *p);
}

int spcbpt_read_local_tone(spcbpt_ctx* c, float* rgba, int* width, int* height) {
    CTX_CHECK(c);
    const Context::LocalTone& b = c->local_last;
    if (!b.have) { c->error = "read_local_tone: no spcbpt_local_tone / spcbpt_local_tone_image since the last spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (c->sync_all()) return SPCBPT_ERR_HIP;
    if (int rc = c->check_diag()) return rc;
    if (width) *width = b.width;
    if (height) *height = b.height;
    if (rgba) HIP_TRY(c, hipMemcpy(rgba, c->d_local, (size_t)b.width * b.height * 16, hipMemcpyDeviceToHost));
    return SPCBPT_OK;
}

}  // extern "C"
