// Context: the bloom stage (kernels_bloom.hip) -- a multi-scale glare of one of the context's linear images or of an image of the
// caller's, into a float4 plane of its own that spcbpt_display can tone-map (SPCBPT_DISPLAY_BLOOM)
// (part of the C ABI library: see capi_common.h for the map of its translation units)
#include "capi_common.h"
#include "kernels_bloom.h"

using namespace spc;

namespace spc {

void Context::free_bloom() {
    d_bloom.release(); d_bloom_pyr.release();
    bloom_last = Plane();
}

static const char* bloom_check(const spcbpt_bloom_params& p) { return bloom_params_error(p.levels, p.strength, p.spread, p.threshold, p.clamp); }

// The launches of one call, on `rstream` between chain_wait and chain_end, one span "bloom".  Down passes for the levels 1 .. j, the
// fused tail from level j (it builds the levels j + 1 .. L and comes back up to U_j inside one workgroup), up passes for j - 1 .. 1, the
// composite.  Without a tail (one level, a coarsest level too large for it, or SPCBPT_BLOOM_TAIL=0; SPCBPT_BLOOM_TAIL=N sets the most
// texels its input level may hold: the developer's switch the cuts were measured with): L down passes, L - 1 up passes, the composite.
// The bits are the same either way.
int Context::bloom_run(const float* src, int width, int height, const spcbpt_bloom_params& p) {
    const size_t px = (size_t)width * height;
    const BloomPlan plan = bloom_plan_of(width, height, p.levels, p.spread);
    HIP_TRY(this, d_bloom.reserve(px * 4));
    HIP_TRY(this, d_bloom_pyr.reserve(plan.texels * 4));
    BloomParams q;
    memset(&q, 0, sizeof(q));
    q.src = src; q.out = d_bloom; q.pyr = d_bloom_pyr;
    q.levels = plan.levels; q.strength = p.strength; q.threshold = p.threshold; q.clamp = p.clamp;
    for (int k = 0; k <= kBloomMaxLevels; k++) { q.w[k] = plan.w[k]; q.h[k] = plan.h[k]; q.off[k] = plan.off[k]; q.g[k] = plan.g[k]; }
    const char* sw = getenv("SPCBPT_BLOOM_TAIL");   // developer: 0 = no tail, N = the tail's input level holds at most N texels
    const int j = sw ? (atoll(sw) > 0 ? bloom_tail_from(q, (size_t)atoll(sw)) : 0) : bloom_tail_from(q);
    const int L = q.levels;
    time_begin("bloom", rstream);
    for (int k = 1; k <= (j ? j : L); k++) launch_bloom_down(q, k, rstream);
    if (j) launch_bloom_tail(q, j, rstream);
    for (int k = (j ? j : L) - 1; k >= 1; k--) launch_bloom_up(q, k, rstream);
    launch_bloom_composite(q, rstream);
    time_end();
    HIP_TRY(this, hipGetLastError());
    bloom_last.have = true; bloom_last.width = width; bloom_last.height = height;
    return 0;
}

// spcbpt_bloom: a link of the film-merge chain like Context::display -- it sees every merge, denoise and resolve queued before it, and
// nothing queued later rewrites its source under it.  Writes its own plane and pyramid only.  The sources and their refusals are
// Context::linear_image's, up to the resolved history image.
int Context::bloom(int source, const spcbpt_bloom_params& p) {
    if (const char* bad = bloom_check(p)) { error = bad; return SPCBPT_ERR_INVALID_ARG; }
    LinearImage im;
    if (int rc = linear_image("bloom", source, SPCBPT_DISPLAY_HISTORY, &im)) return rc;
    return chain_link([&] { return bloom_run(im.p, im.width, im.height, p); });
}

// spcbpt_bloom_image: the same link over the scratch copy of the caller's image (Context::image_link).
int Context::bloom_image(const float* rgba, int width, int height, const spcbpt_bloom_params& p) {
    if (const char* bad = bloom_check(p)) { error = bad; return SPCBPT_ERR_INVALID_ARG; }
    if (int rc = caller_image("bloom", rgba, width, height)) return rc;
    return image_link(rgba, width, height, [&](const float* src) { return bloom_run(src, width, height, p); });
}

}  // namespace spc

extern "C" {

int spcbpt_bloom(spcbpt_ctx* c, int source, const spcbpt_bloom_params* p) {
    CTX_CHECK(c);
    if (!p) { c->error = "null params"; return SPCBPT_ERR_INVALID_ARG; }
    return c->bloom(source, *p);
}

int spcbpt_bloom_image(spcbpt_ctx* c, const float* rgba, int width, int height, const spcbpt_bloom_params* p) {
    CTX_CHECK(c);
    if (!p) { c->error = "null params"; return SPCBPT_ERR_INVALID_ARG; }
    return c->bloom_image(rgba, width, height, *p);
}

int spcbpt_read_bloom(spcbpt_ctx* c, float* rgba, int* width, int* height) {
    CTX_CHECK(c);
    return c->read_plane("bloom", c->bloom_last, c->d_bloom, rgba, width, height);
}

}  // extern "C"
