// Context: the display transform (kernels_display.hip) -- exposure, histogram auto-exposure and the tone operators over one of the
// context's linear images or an image of the caller's, into an RGBA8 plane of its own -- and what the bloom and the local tone stage
// share with it: the sources (Context::linear_image) and the scratch copy of a caller's image
// (part of the C ABI library: see capi_common.h for the map of its translation units)
#include "capi_common.h"
#include "kernels_display.h"

using namespace spc;

namespace spc {

void Context::free_display() {
    d_display_frame.release(); d_display_state.release(); d_stage_src.release();
    display_last = Display();
}

static const char* display_check(const spcbpt_display_params& p) {
    return display_params_error(p.op, p.flags, p.ev, p.key, p.low_fraction, p.high_fraction, p.ev_bias, p.ev_min, p.ev_max, p.adapt, p.white);
}

// The launches of one call, on `rstream` between chain_wait and chain_end.  Manual exposure: k_display_map alone.  Auto: a memset of the
// counters, the histogram, the exposure kernel, the map -- the EV goes from kernel to kernel through the record and the host never
// waits for it.  SPCBPT_DISPLAY_HISTOGRAM runs the first two under manual exposure as well.  Spans: "display_hist", "display".
int Context::display_run(const float* src, int width, int height, const spcbpt_display_params& p) {
    const size_t px = (size_t)width * height;
    const bool auto_ev = (p.flags & SPCBPT_DISPLAY_AUTO) != 0, hist = auto_ev || (p.flags & SPCBPT_DISPLAY_HISTOGRAM) != 0;
    HIP_TRY(this, d_display_frame.reserve(px));
    if (hist && !d_display_state) {   // the record: counters and adaptation state, zero = no previous EV
        HIP_TRY(this, d_display_state.reserve(kDisplayStateWords));
        HIP_TRY(this, hipMemsetAsync(d_display_state, 0, kDisplayStateWords * sizeof(uint32_t), rstream));
    }
    DisplayParams q;
    memset(&q, 0, sizeof(q));
    q.pixels = px; q.src = src; q.frame = d_display_frame; q.state = d_display_state;
    q.op = p.op; q.auto_ev = auto_ev ? 1 : 0; q.ev = p.ev; q.white = p.white;
    q.exposure = display_exposure_of(p.key, p.low_fraction, p.high_fraction, p.ev_bias, p.ev_min, p.ev_max, p.adapt);
    if (hist) {
        time_begin("display_hist", rstream);
        HIP_TRY(this, hipMemsetAsync(d_display_state, 0, kDisplayCounters * sizeof(uint32_t), rstream));
        launch_display_histogram(q, rstream);
        if (auto_ev) launch_display_exposure(q, rstream);
        time_end();
    }
    time_begin("display", rstream);
    launch_display_map(q, rstream);
    time_end();
    HIP_TRY(this, hipGetLastError());
    display_last.have = true; display_last.have_hist = hist; display_last.auto_ev = auto_ev;
    display_last.width = width; display_last.height = height; display_last.ev = p.ev;
    return 0;
}

// A source of the image-space stages as a pointer and a size, or the stage's refusal under its name `who`: the range (a stage takes the
// sources up to its `last_source`), the deferred frame, the film for the four sources of its size, the plane itself.  The bloom and the
// local tone plane come at the size of the image they were made from and need no film (spcbpt_bloom_image needs none).
int Context::linear_image(const char* who, int source, int last_source, LinearImage* out) {
    struct Row { int source; const char* name; bool have; const float* p; const Plane* size; const char* missing; };   // size: null = the film's
    const Row rows[] = {
        {SPCBPT_DISPLAY_FILM, "film", true, d_accum, nullptr, ""},
        {SPCBPT_DISPLAY_DENOISED, "denoised", have_denoised, d_denoised, nullptr, "no denoised image: spcbpt_denoise / spcbpt_denoise_variance / spcbpt_history_denoise since the last spcbpt_resize"},
        {SPCBPT_DISPLAY_ROBUST, "robust", film_buckets && have_robust, d_robust, nullptr,
         !film_buckets ? "no robust image: the film's buckets are off (spcbpt_set_film_buckets, then spcbpt_robust_resolve)" : "no robust image: no spcbpt_robust_resolve since the film's buckets were last set up"},
        {SPCBPT_DISPLAY_HISTORY, "history", have_resolved, d_resolved, nullptr, "no resolved history image: spcbpt_history_resolve since the last spcbpt_resize / spcbpt_history_reset"},
        {SPCBPT_DISPLAY_BLOOM, "bloom", bloom_last.have, d_bloom, &bloom_last, "no bloom plane: spcbpt_bloom / spcbpt_bloom_image since the last spcbpt_resize"},
        {SPCBPT_DISPLAY_LOCAL, "local", local_last.have, d_local, &local_last, "no local tone plane: spcbpt_local_tone / spcbpt_local_tone_image since the last spcbpt_resize"},
    };
    static_assert(SPCBPT_DISPLAY_FILM == 0 && SPCBPT_DISPLAY_LOCAL == sizeof(rows) / sizeof(rows[0]) - 1, "rows[source] is the row of `source`");
    const std::string stage = who;
    if (source < 0 || source > last_source) {
        error = stage + ": source must be ";   // "0 (film), 1 (denoised), 2 (robust) or 3 (history)"
        for (int k = 0; k <= last_source; k++) error += (k == 0 ? "" : k == last_source ? " or " : ", ") + std::to_string(rows[k].source) + " (" + rows[k].name + ")";
        return SPCBPT_ERR_INVALID_ARG;
    }
    if (deferred.active) { error = stage + ": a deferred frame is outstanding: spcbpt_merge_deferred(ctx, keep) first"; return SPCBPT_ERR_STATE; }
    const Row& r = rows[source];
    if (!r.size && !d_accum) { error = stage + " before spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (!r.have) { error = stage + ": " + r.missing; return SPCBPT_ERR_STATE; }
    *out = r.size ? LinearImage{r.p, r.size->width, r.size->height} : LinearImage{r.p, (int)kp.width, (int)kp.height};
    return 0;
}

// spcbpt_*_image: the caller's image is there and holds 1 .. 2^28 pixels ...
int Context::caller_image(const char* who, const float* rgba, int width, int height) {
    if (!rgba) { error = "null pointer"; return SPCBPT_ERR_INVALID_ARG; }
    if (width < 1 || height < 1 || (int64_t)width * height > (1ll << 28)) { error = std::string(who) + "_image: the image must hold 1 .. 2^28 pixels"; return SPCBPT_ERR_INVALID_ARG; }
    return 0;
}

// ... and its scratch copy (Context::image_link).  The upload is queued behind the chain (the link before may still read the scratch)
// and waited for, so that the caller's image may go when the call returns.
int Context::stage_upload(const float* rgba, int width, int height) {
    const size_t px = (size_t)width * height;
    HIP_TRY(this, d_stage_src.reserve(px * 4));
    HIP_TRY(this, hipMemcpyAsync(d_stage_src, rgba, px * 16, hipMemcpyHostToDevice, rstream));
    HIP_TRY(this, hipStreamSynchronize(rstream));
    return 0;
}

// spcbpt_read_bloom / spcbpt_read_local_tone: the float4 plane of `stage` and its size, each optional.
int Context::read_plane(const char* stage, const Plane& b, const float* plane, float* rgba, int* width, int* height) {
    if (!b.have) { error = std::string("read_") + stage + ": no spcbpt_" + stage + " / spcbpt_" + stage + "_image since the last spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (sync_all()) return SPCBPT_ERR_HIP;
    if (int rc = check_diag()) return rc;
    if (width) *width = b.width;
    if (height) *height = b.height;
    if (rgba) HIP_TRY(this, hipMemcpy(rgba, plane, (size_t)b.width * b.height * 16, hipMemcpyDeviceToHost));
    return SPCBPT_OK;
}

// spcbpt_display: a link of the film-merge chain like Context::robust_resolve -- it sees every merge, denoise and resolve queued before
// it, and nothing queued later rewrites its source under it.  Writes its own plane and record only.
int Context::display(int source, const spcbpt_display_params& p) {
    if (const char* bad = display_check(p)) { error = bad; return SPCBPT_ERR_INVALID_ARG; }
    LinearImage im;
    if (int rc = linear_image("display", source, SPCBPT_DISPLAY_LOCAL, &im)) return rc;
    return chain_link([&] { return display_run(im.p, im.width, im.height, p); });
}

// spcbpt_display_image: the same link over the scratch copy of the caller's image; nothing waits for the EV.
int Context::display_image(const float* rgba, int width, int height, const spcbpt_display_params& p) {
    if (const char* bad = display_check(p)) { error = bad; return SPCBPT_ERR_INVALID_ARG; }
    if (int rc = caller_image("display", rgba, width, height)) return rc;
    return image_link(rgba, width, height, [&](const float* src) { return display_run(src, width, height, p); });
}

// spcbpt_display_reset: the record's adaptation words to zero, as a chain link: behind the display calls already queued.
int Context::display_reset() {
    if (!d_display_state) return 0;   // no auto call yet: nothing to forget
    next_render_stream();
    if (int rc = chain_wait()) return rc;
    HIP_TRY(this, hipMemsetAsync(d_display_state.p + kDisplayStateEv, 0, 2 * sizeof(uint32_t), rstream));
    return chain_end();
}

}  // namespace spc

extern "C" {

int spcbpt_display(spcbpt_ctx* c, int source, const spcbpt_display_params* p) {
    CTX_CHECK(c);
    if (!p) { c->error = "null params"; return SPCBPT_ERR_INVALID_ARG; }
    return c->display(source, *p);
}

int spcbpt_display_image(spcbpt_ctx* c, const float* rgba, int width, int height, const spcbpt_display_params* p) {
    CTX_CHECK(c);
    if (!p) { c->error = "null params"; return SPCBPT_ERR_INVALID_ARG; }
    return c->display_image(rgba, width, height, *p);
}

int spcbpt_display_reset(spcbpt_ctx* c) {
    CTX_CHECK(c);
    return c->display_reset();
}

int spcbpt_read_display(spcbpt_ctx* c, uint8_t* rgba8, uint32_t* histogram258, float* ev, int* width, int* height) {
    CTX_CHECK(c);
    const Context::Display& d = c->display_last;
    if (!d.have) { c->error = "read_display: no spcbpt_display / spcbpt_display_image since the last spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (histogram258 && !d.have_hist) { c->error = "read_display: the last display call computed no histogram (manual exposure without SPCBPT_DISPLAY_HISTOGRAM)"; return SPCBPT_ERR_STATE; }
    if (c->sync_all()) return SPCBPT_ERR_HIP;
    if (int rc = c->check_diag()) return rc;
    if (width) *width = d.width;
    if (height) *height = d.height;
    if (rgba8) HIP_TRY(c, hipMemcpy(rgba8, c->d_display_frame, (size_t)d.width * d.height * 4, hipMemcpyDeviceToHost));
    if (histogram258) HIP_TRY(c, hipMemcpy(histogram258, c->d_display_state, kDisplayCounters * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (ev) {
        if (d.auto_ev) HIP_TRY(c, hipMemcpy(ev, c->d_display_state.p + kDisplayStateEv, sizeof(float), hipMemcpyDeviceToHost));
        else *ev = d.ev;
    }
    return SPCBPT_OK;
}

}  // extern "C"
