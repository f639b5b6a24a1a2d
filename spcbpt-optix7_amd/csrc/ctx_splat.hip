// Context: the light-tracing launch "lt" (kernels_splat.hip), and the exported camera projection it shares with the kernel
// (part of the C ABI library: see capi_common.h for the map of its translation units)
#include "capi_common.h"
#include "dev_splat.h"
#include "kernels_splat.h"

using namespace spc;

namespace spc {

// spcbpt_launch(ctx, "lt", ...): the cache of the sampler set an eye launch would read (`eset`), splatted onto the rows of the band
// set and merged into the film as this subframe.  Stream and event discipline are launch_render's: the launch takes the next render
// stream, waits for the set's sampler build, and records sets[eset].render so that no later light pass rewrites the set under it.
// Event counters (spcbpt_enable_counters) are left untouched: the splat kernel charges none.
int Context::launch_splat(uint32_t frame, int r0, int r1, int rs) {
    int rc = uniform_merge_allowed("lt");
    if (rc) return rc;
    if ((rc = film_ready())) return rc;
    if (kp.scene.env.valid) {
        error = "lt: not with an environment map: the directly seen sky is not sampled by this estimator, and the sky vertices of the cache "
                "(SPCBPT_LV_DIRECTION) have no position to project";
        return SPCBPT_ERR_STATE;
    }
    if (!have_sampler) { error = "lt needs a built sampler (\"light trace\" -> spcbpt_build_sampler)"; return SPCBPT_ERR_STATE; }
    if ((rc = begin_render(r0, r1, rs))) return rc;
    kp.subframe = frame;
    kp.result = d_result[rk];
    if (rstream != stream) HIP_TRY(this, sets[eset].sampler.wait_on(rstream));
    const size_t px = (size_t)kp.width * kp.height;
    const bool ordered = splat_order == SPCBPT_SPLAT_ORDERED;
    const int capacity = (int)std::min<size_t>(lvc_capacity, 0x7fffffff);
    if (!ordered) {
        // the splat buffer of this render stream: allocated at the first atomic "lt" launch after a resize, so that a context that never
        // launches "lt" keeps its footprint (spcbpt_resize has synchronised every stream before the size changed)
        if (d_splat[rk].cap != px * 4) d_splat[rk].release();   // (not grow-only: a smaller film gets a smaller buffer)
        HIP_TRY(this, d_splat[rk].reserve(px * 4));
    }
    const int threads = splat_block_threads();
    const int blocks = splat_blocks(std::min(4 * std::max(1, num_cus), (capacity + threads - 1) / threads));
    rc = ensure_spill((size_t)blocks * (size_t)threads, true);
    if (rc) return rc;
    SplatParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.scene = kp.scene;
    memcpy(sp.eye, kp.eye, 12); memcpy(sp.U, kp.U, 12); memcpy(sp.V, kp.V, 12); memcpy(sp.W, kp.W, 12);
    sp.width = kp.width; sp.height = kp.height; sp.subframe = kp.subframe;
    sp.row_begin = kp.row_begin; sp.row_end = kp.row_end; sp.row_step = kp.row_step;
    sp.lvc = sets[eset].lvc; sp.sampler_counts = sets[eset].counts; sp.capacity = capacity;
    sp.splat = d_splat[rk]; sp.result = kp.result;
    sp.spill = kp.spill; sp.spill_entries = kp.spill_entries; sp.diag = kp.diag;
    sp.lens_radius = kp.lens_radius; sp.lens_focus = kp.lens_focus; memcpy(sp.lens_u, kp.lens_u, 12); memcpy(sp.lens_v, kp.lens_v, 12);   // spcbpt_set_lens: radius > 0 selects the lens kernels (kernels_splat.hip)
    if (!ordered) {
        HIP_TRY(this, hipMemsetAsync(d_splat[rk], 0, px * 16, rstream));
        time_begin("lt", rstream);
        launch_lt_splat(sp, blocks, rstream);
        launch_lt_resolve(sp, rstream);
        time_end();
    } else {
        // Ordered: records -> stable radix sort of (pixel, slot) over `bound` slots -> per-pixel sum in slot order.  The buffers are
        // sized by the cache capacity (grow-only: a reallocation's hipFree waits for the device by itself), the passes by `bound`.
        SplatOrdered& O = d_ordered[rk];
        const int bound = splat_bound(capacity);
        int key_bits = 1;
        while (key_bits < 32 && ((uint64_t)1 << key_bits) <= (uint64_t)px) key_bits++;   // ceil(log2(pixels + 1)): the pad key `pixels` has its bits
        const size_t slots = (size_t)std::max(capacity, 1);
        HIP_TRY(this, O.records.reserve(slots * 4));
        HIP_TRY(this, O.keys.reserve(slots)); HIP_TRY(this, O.vals.reserve(slots));
        HIP_TRY(this, O.keys2.reserve(slots)); HIP_TRY(this, O.vals2.reserve(slots));
        HIP_TRY(this, O.count.reserve(1));
        size_t tb = 0;
        if (bound > 0) {
            HIP_TRY(this, hipcub::DeviceRadixSort::SortPairs(nullptr, tb, O.keys.p, O.keys2.p, O.vals.p, O.vals2.p, bound, 0, key_bits, rstream));
            HIP_TRY(this, O.temp.reserve(tb));
        }
        sp.records = reinterpret_cast<float4*>(O.records.p); sp.keys = O.keys; sp.vals = O.vals;
        sp.keys_sorted = O.keys2; sp.vals_sorted = O.vals2; sp.bound = bound;
        time_begin("lt", rstream);
        launch_lt_records(sp, blocks, rstream);
        hipError_t sorted = hipSuccess;
        if (bound > 0) sorted = hipcub::DeviceRadixSort::SortPairs(O.temp.p, tb, O.keys.p, O.keys2.p, O.vals.p, O.vals2.p, bound, 0, key_bits, rstream);
        if (sorted == hipSuccess) launch_lt_gather(sp, rstream);
        time_end();
        HIP_TRY(this, sorted);
        // what spcbpt_read_splat_records needs of this launch: the count the kernels read, taken before render_done lets a light pass at the set
        HIP_TRY(this, hipMemcpyAsync(O.count.p, sets[eset].counts, sizeof(int), hipMemcpyDeviceToDevice, rstream));
        splat_records_rk = rk; splat_records_capacity = bound; splat_records_pixels = (int)px;
    }
    HIP_TRY(this, hipGetLastError());
    rc = render_done(eset);
    return rc ? rc : finish_frame();
}

// An upper bound of the vertex count of set `eset` that the host has WITHOUT waiting: the count an import told it, or the one the
// set's light pass has left in pinned memory if that pass is already over (an event query, no wait); otherwise the set's capacity.
// The film does not depend on which it is: slots past the device's own count get the pad key, which no pixel owns.
int Context::splat_bound(int capacity) {
    const CacheSet& S = sets[eset];
    int n = capacity;
    if (S.count_host >= 0) n = S.count_host;
    else if (S.bound >= 0) n = S.bound;
    else if (S.light_counts_valid && S.light.set) {
        if (hipEventQuery(S.light.ev) == hipSuccess) n = h_light_counts[2 * eset];
        else (void)hipGetLastError();   // hipErrorNotReady is no failure of this launch
    }
    return std::max(0, std::min(n, capacity));
}

int Context::set_splat_order(int mode) {
    if (mode != SPCBPT_SPLAT_ATOMIC && mode != SPCBPT_SPLAT_ORDERED) { error = "set_splat_order: mode must be SPCBPT_SPLAT_ATOMIC (0) or SPCBPT_SPLAT_ORDERED (1)"; return SPCBPT_ERR_INVALID_ARG; }
    if (deferred.active) { error = "a deferred frame is outstanding: spcbpt_merge_deferred(ctx, keep) first"; return SPCBPT_ERR_STATE; }
    if (mode == splat_order) return 0;
    if (mode == SPCBPT_SPLAT_ATOMIC) {   // the buffers go with the mode: launches that still use them may be queued
        if (sync_all()) return SPCBPT_ERR_HIP;
        for (SplatOrdered& O : d_ordered) O.release();
        splat_records_rk = -1;
    }
    splat_order = mode;
    return 0;
}

int Context::read_splat_records(float* rgb, int32_t* pixel, int capacity, int* count) {
    if (splat_records_rk < 0) { error = "read_splat_records: no ordered \"lt\" launch since the last spcbpt_resize (spcbpt_set_splat_order(ctx, SPCBPT_SPLAT_ORDERED), then launch \"lt\")"; return SPCBPT_ERR_STATE; }
    if (sync_all()) return SPCBPT_ERR_HIP;
    if (int rc = check_diag()) return rc;
    const SplatOrdered& O = d_ordered[splat_records_rk];
    int n = 0;
    HIP_TRY(this, hipMemcpy(&n, O.count.p, sizeof(int), hipMemcpyDeviceToHost));
    n = std::max(0, std::min(n, splat_records_capacity));   // what k_lt_records took as the cache's vertex count
    *count = n;
    if (capacity < n || (n > 0 && (!rgb || !pixel))) { error = "read_splat_records: buffer too small"; return SPCBPT_ERR_CAPACITY; }
    if (n == 0) return SPCBPT_OK;
    std::vector<float> rec((size_t)n * 4);
    HIP_TRY(this, hipMemcpy(rec.data(), O.records.p, rec.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) {
        uint32_t key;
        memcpy(&key, &rec[(size_t)i * 4 + 3], 4);
        const bool none = key >= (uint32_t)splat_records_pixels;   // the pad key
        pixel[i] = none ? -1 : (int32_t)key;
        for (int k = 0; k < 3; k++) rgb[(size_t)i * 3 + k] = none ? 0.0f : rec[(size_t)i * 4 + k];
    }
    return SPCBPT_OK;
}

}  // namespace spc

extern "C" int spcbpt_set_splat_order(spcbpt_ctx* c, int mode) {
    CTX_CHECK(c);
    return c->set_splat_order(mode);
}
extern "C" int spcbpt_get_splat_order(spcbpt_ctx* c, int* mode) {
    CTX_CHECK(c);
    if (!mode) { c->error = "null pointer"; return SPCBPT_ERR_INVALID_ARG; }
    *mode = c->splat_order;
    return SPCBPT_OK;
}
extern "C" int spcbpt_read_splat_records(spcbpt_ctx* c, float* rgb, int32_t* pixel, int capacity, int* count) {
    CTX_CHECK(c);
    if (!count) { c->error = "null pointer"; return SPCBPT_ERR_INVALID_ARG; }
    return c->read_splat_records(rgb, pixel, capacity, count);
}

extern "C" int spcbpt_camera_splat(const float eye[3], const float U[3], const float V[3], const float W[3], int width, int height,
                                   const float point[3], float* dx, float* dy, int* px, int* py, float* weight) {
    if (!eye || !U || !V || !W || !point || width < 1 || height < 1) return 0;
    float x, y, we;
    int ix, iy;
    if (!camera_splat(eye, U, V, W, width, height, point, x, y, ix, iy, we)) return 0;
    if (dx) *dx = x;
    if (dy) *dy = y;
    if (px) *px = ix;
    if (py) *py = iy;
    if (weight) *weight = we;
    return 1;
}
