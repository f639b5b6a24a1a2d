// Context: the bucket film (kernels_buckets.hip) -- K per-pixel bucket means in front of every film merge of finish_frame -- and the
// median-of-means resolve that reads them
// (part of the C ABI library: see capi_common.h for the map of its translation units)
#include "capi_common.h"
#include "kernels_buckets.h"

using namespace spc;

namespace spc {

void Context::free_buckets() {
    d_buckets.release(); d_robust.release(); d_robust_frame.release();
    have_robust = false;
}

int Context::set_film_buckets(int k) {
    if (k != 0 && !film_buckets_valid(k)) { error = "set_film_buckets: the number of buckets must be 0 (off) or 3 .. 32"; return SPCBPT_ERR_INVALID_ARG; }
    if (k == film_buckets) return 0;
    if (adaptive.active) { error = "set_film_buckets: adaptive sampling is active and its per-tile merge keeps no buckets: spcbpt_adaptive_end first"; return SPCBPT_ERR_STATE; }
    if (film_buckets) {   // the planes go with the switch and with K: merges that still write them may be queued
        if (sync_all()) return SPCBPT_ERR_HIP;
        free_buckets();
    }
    film_buckets = k;
    return 0;
}

// the planes: allocated (and zeroed, for the rows a banded launch leaves alone) at the first merge or resolve after a resize
int Context::ensure_buckets(hipStream_t s) {
    if (d_buckets) return 0;
    const size_t px = (size_t)kp.width * kp.height;
    HIP_TRY(this, d_buckets.reserve(px * 4 * (size_t)film_buckets));
    HIP_TRY(this, hipMemsetAsync(d_buckets, 0, px * 16 * (size_t)film_buckets, s));
    return 0;
}

// finish_frame, after chain_wait and in front of launch_film_merge on the same stream (beside moments_step, independent of it): the
// frame's samples into bucket subframe % K of the pixels this launch's merge rewrites.  The kernel-time span is "buckets".
int Context::buckets_step() {
    if (int rc = ensure_buckets(rstream)) return rc;
    BucketParams bp;
    memset(&bp, 0, sizeof(bp));
    bp.width = kp.width; bp.height = kp.height; bp.subframe = kp.subframe;
    bp.row_begin = kp.row_begin; bp.row_end = kp.row_end; bp.row_step = kp.row_step;
    bp.buckets = film_buckets; bp.result = kp.result; bp.planes = d_buckets;
    time_begin("buckets", rstream);
    launch_film_buckets(bp, rstream);
    time_end();
    HIP_TRY(this, hipGetLastError());
    return 0;
}

// spcbpt_robust_resolve: one launch, a link of the film-merge chain like Context::denoise -- it sees every merge queued before it and no
// later merge rewrites the buckets under it.  Writes its own two planes only.  The kernel-time span is "robust_resolve".
int Context::robust_resolve(float strength) {
    if (!film_buckets) { error = "robust_resolve needs the film's buckets: spcbpt_set_film_buckets(ctx, K) before the frames are rendered"; return SPCBPT_ERR_STATE; }
    if (deferred.active) { error = "a deferred frame is outstanding: spcbpt_merge_deferred(ctx, keep) first"; return SPCBPT_ERR_STATE; }
    if (!d_accum) { error = "robust_resolve before spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (!(strength >= 0.0f && strength <= 8.0f)) { error = "robust_resolve: strength must be a number in [0, 8]"; return SPCBPT_ERR_INVALID_ARG; }
    next_render_stream();
    if (int rc = chain_wait()) return rc;
    if (int rc = ensure_buckets(rstream)) return rc;   // buckets on, but no merge since the last resize: every bucket has n = 0
    const size_t px = (size_t)kp.width * kp.height;
    if (!d_robust) {
        HIP_TRY(this, d_robust_frame.reserve(px));
        HIP_TRY(this, d_robust.reserve(px * 4));
    }
    RobustParams q;
    memset(&q, 0, sizeof(q));
    q.width = kp.width; q.height = kp.height; q.buckets = film_buckets; q.strength = strength;
    q.planes = d_buckets; q.out = d_robust; q.frame = d_robust_frame;
    time_begin("robust_resolve", rstream);
    launch_robust_resolve(q, rstream);
    time_end();
    HIP_TRY(this, hipGetLastError());
    have_robust = true;
    return chain_end();
}

}  // namespace spc

extern "C" {

int spcbpt_set_film_buckets(spcbpt_ctx* c, int buckets) {
    CTX_CHECK(c);
    return c->set_film_buckets(buckets);
}
int spcbpt_get_film_buckets(spcbpt_ctx* c, int* buckets) {
    CTX_CHECK(c);
    if (!buckets) { c->error = "null pointer"; return SPCBPT_ERR_INVALID_ARG; }
    *buckets = c->film_buckets;
    return SPCBPT_OK;
}

int spcbpt_read_film_buckets(spcbpt_ctx* c, float* out) {
    CTX_CHECK(c);
    if (!c->film_buckets) { c->error = "read_film_buckets: the film's buckets are off (spcbpt_set_film_buckets)"; return SPCBPT_ERR_STATE; }
    if (!c->d_accum) { c->error = "read_film_buckets before spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (!out) { c->error = "null pointer"; return SPCBPT_ERR_INVALID_ARG; }
    if (c->sync_all()) return SPCBPT_ERR_HIP;
    if (int rc = c->check_diag()) return rc;
    const size_t bytes = (size_t)c->kp.width * c->kp.height * 16 * (size_t)c->film_buckets;
    if (!c->d_buckets) { memset(out, 0, bytes); return SPCBPT_OK; }   // no merge since the last resize
    HIP_TRY(c, hipMemcpy(out, c->d_buckets, bytes, hipMemcpyDeviceToHost));
    return SPCBPT_OK;
}

int spcbpt_robust_resolve(spcbpt_ctx* c, float strength) {
    CTX_CHECK(c);
    return c->robust_resolve(strength);
}

int spcbpt_read_robust(spcbpt_ctx* c, float* rgba, uint32_t* frame) {
    CTX_CHECK(c);
    if (!c->film_buckets) { c->error = "read_robust: the film's buckets are off (spcbpt_set_film_buckets)"; return SPCBPT_ERR_STATE; }
    if (!c->have_robust) { c->error = "read_robust: no spcbpt_robust_resolve since the film's buckets were last set up (spcbpt_resize, spcbpt_set_film_buckets)"; return SPCBPT_ERR_STATE; }
    if (c->sync_all()) return SPCBPT_ERR_HIP;
    if (int rc = c->check_diag()) return rc;
    const size_t px = (size_t)c->kp.width * c->kp.height;
    if (rgba) HIP_TRY(c, hipMemcpy(rgba, c->d_robust, px * 16, hipMemcpyDeviceToHost));
    if (frame) HIP_TRY(c, hipMemcpy(frame, c->d_robust_frame, px * 4, hipMemcpyDeviceToHost));
    return SPCBPT_OK;
}

}  // extern "C"
