// Context: the local tone stage (kernels_local_tone.hip) -- a base / detail decomposition of log-luminance through a bilateral grid, of
// one of the context's linear images, of the bloom plane or of an image of the caller's, into a float4 plane of its own that
// spcbpt_display can tone-map (SPCBPT_DISPLAY_LOCAL)
// (part of the C ABI library: see capi_common.h for the map of its translation units)
#include "capi_common.h"
#include "kernels_local_tone.h"

using namespace spc;

namespace spc {

void Context::free_local_tone() {
    d_local.release(); d_local_grid[0].release(); d_local_grid[1].release();
    local_last = Plane();
}

static const char* local_tone_check(const spcbpt_local_tone_params& p) { return local_tone_params_error(p.cell, p.range, p.blur, p.compress, p.detail, p.anchor); }
// ... and of the grid an image of this size would need, once the size is known and before the link begins
static const char* local_tone_grid_check(int width, int height, const spcbpt_local_tone_params& p) {
    return local_tone_plan_of(width, height, p.cell, p.range, p.anchor).nodes > kLtMaxNodes ? "local_tone: the grid would have more than 2^25 nodes: a larger cell or range" : nullptr;
}

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
// it, and nothing queued later rewrites its source under it.  Writes its own plane and grid buffers only.  The sources and their
// refusals are Context::linear_image's, up to the bloom plane.
int Context::local_tone(int source, const spcbpt_local_tone_params& p) {
    if (const char* bad = local_tone_check(p)) { error = bad; return SPCBPT_ERR_INVALID_ARG; }
    LinearImage im;
    if (int rc = linear_image("local_tone", source, SPCBPT_DISPLAY_BLOOM, &im)) return rc;
    if (const char* bad = local_tone_grid_check(im.width, im.height, p)) { error = bad; return SPCBPT_ERR_INVALID_ARG; }
    return chain_link([&] { return local_tone_run(im.p, im.width, im.height, p); });
}

// spcbpt_local_tone_image: the same link over the scratch copy of the caller's image (Context::image_link).
int Context::local_tone_image(const float* rgba, int width, int height, const spcbpt_local_tone_params& p) {
    if (const char* bad = local_tone_check(p)) { error = bad; return SPCBPT_ERR_INVALID_ARG; }
    if (int rc = caller_image("local_tone", rgba, width, height)) return rc;
    if (const char* bad = local_tone_grid_check(width, height, p)) { error = bad; return SPCBPT_ERR_INVALID_ARG; }
    return image_link(rgba, width, height, [&](const float* src) { return local_tone_run(src, width, height, p); });
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
    return c->read_plane("local_tone", c->local_last, c->d_local, rgba, width, height);
}

}  // extern "C"
