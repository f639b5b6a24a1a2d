// Context: adaptive sampling -- the per-tile sample counts, the tile errors and the tile list (kernels_adaptive.hip), the eye
// megakernel fed from the list (kernels.hip: k_spcbpt_tiles) and the merge of the listed tiles
// (part of the C ABI library: see capi_common.h for the map of its translation units)
#include "capi_common.h"
#include "kernels_adaptive.h"

using namespace spc;

namespace spc {

int Context::uniform_merge_allowed(const char* what) {
    if (!adaptive.active) return 0;
    error = std::string(what) + ": adaptive sampling is active (spcbpt_adaptive_begin): the film's tiles stand at sample counts of their own, and this launch "
            "merges with one weight for all pixels -- spcbpt_launch_adaptive, or spcbpt_adaptive_end first";
    return SPCBPT_ERR_STATE;
}

void Context::adaptive_drop() {
    adaptive.active = false;
    adaptive.tiles_x = adaptive.tiles_y = adaptive.n_listed = 0;
    adaptive.samples.release(); adaptive.known.release(); adaptive.list.release(); adaptive.n_dev.release(); adaptive.error.release();
}

int Context::adaptive_begin(uint32_t frames) {
    if (deferred.active) { error = "adaptive_begin: a deferred frame is outstanding: spcbpt_merge_deferred(ctx, keep) first"; return SPCBPT_ERR_STATE; }
    if (!d_accum) { error = "adaptive_begin before spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (!film_moments) { error = "adaptive_begin needs the film's moments: spcbpt_set_film_moments(ctx, 1) before the frames are rendered"; return SPCBPT_ERR_STATE; }
    if (film_buckets) { error = "adaptive_begin: not with the film's buckets on (spcbpt_set_film_buckets): the per-tile merge fills no buckets"; return SPCBPT_ERR_STATE; }
    if (kp.width >= 65536u || kp.height >= 65536u) { error = "adaptive_begin: image too large"; return SPCBPT_ERR_INVALID_ARG; }
    if (sync_all()) return SPCBPT_ERR_HIP;
    const int tx = (int)adaptive_tiles_x(kp.width), ty = (int)adaptive_tiles_y(kp.height);
    const size_t n = (size_t)tx * ty;
    HIP_TRY(this, adaptive.samples.reserve(n));
    HIP_TRY(this, adaptive.known.reserve(n));
    HIP_TRY(this, adaptive.list.reserve(n));
    HIP_TRY(this, adaptive.error.reserve(n));
    HIP_TRY(this, adaptive.n_dev.reserve(1));
    HIP_TRY(this, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(adaptive.samples.p), (int)frames, n, rstream));
    HIP_TRY(this, hipMemsetAsync(adaptive.known, 0, n * 4, rstream));
    HIP_TRY(this, hipMemsetAsync(adaptive.error, 0, n * 4, rstream));
    HIP_TRY(this, hipMemsetAsync(adaptive.n_dev, 0, 4, rstream));
    HIP_TRY(this, hipStreamSynchronize(rstream));
    adaptive.tiles_x = tx; adaptive.tiles_y = ty; adaptive.n_listed = 0;
    adaptive.active = true;
    return 0;
}

// Two launches behind the last merge queued, on that merge's stream (every adaptive launch before it ends in a merge of the chain, so
// nothing still reads the list that is rewritten), and a read-back of 4 bytes.  The kernel-time span is "adaptive_select".
int Context::adaptive_select(const spcbpt_adaptive_params& ap, int* n_selected) {
    if (!adaptive.active) { error = "adaptive_select: adaptive sampling is not active (spcbpt_adaptive_begin)"; return SPCBPT_ERR_STATE; }
    if (!(ap.target_error == ap.target_error)) { error = "adaptive_select: target_error is not a number"; return SPCBPT_ERR_INVALID_ARG; }
    const size_t px = (size_t)kp.width * kp.height;
    const uint32_t n_tiles = (uint32_t)(adaptive.tiles_x * adaptive.tiles_y);
    hipStream_t s = last_merge_k >= 0 ? rstreams[last_merge_k] : rstream;
    if (!d_m2n) {   // moments on, but no merge since the last resize: every pixel has n = 0
        HIP_TRY(this, d_m2n.reserve(px * 4));
        HIP_TRY(this, hipMemsetAsync(d_m2n, 0, px * 16, s));
    }
    time_begin("adaptive_select", s);
    launch_tile_error(d_accum, d_m2n, kp.width, kp.height, adaptive.error, adaptive.known, s);
    launch_tile_select(adaptive.error, adaptive.known, adaptive.samples, n_tiles, ap.target_error, ap.min_samples, ap.max_samples, adaptive.list, adaptive.n_dev, s);
    time_end();
    HIP_TRY(this, hipGetLastError());
    uint32_t n = 0;
    HIP_TRY(this, hipMemcpyAsync(&n, adaptive.n_dev, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(this, hipStreamSynchronize(s));
    if (n > n_tiles) { error = "adaptive_select: the device returned a list longer than the film has tiles"; adaptive.n_listed = 0; return SPCBPT_ERR_STATE; }
    adaptive.n_listed = (int)n;
    if (n_selected) *n_selected = (int)n;
    return check_diag();
}

int Context::adaptive_set_tiles(const uint32_t* tiles, int n) {
    if (!adaptive.active) { error = "adaptive_set_tiles: adaptive sampling is not active (spcbpt_adaptive_begin)"; return SPCBPT_ERR_STATE; }
    const int n_tiles = adaptive.tiles_x * adaptive.tiles_y;
    if (n < 0 || n > n_tiles || (n > 0 && !tiles)) { error = "adaptive_set_tiles: 0 .. tiles_x * tiles_y tiles"; return SPCBPT_ERR_INVALID_ARG; }
    for (int i = 0; i < n; i++) {
        if (tiles[i] >= (uint32_t)n_tiles) { error = "adaptive_set_tiles: tile " + std::to_string(tiles[i]) + " is out of range (the film has " + std::to_string(n_tiles) + " tiles)"; return SPCBPT_ERR_INVALID_ARG; }
        if (i > 0 && tiles[i] <= tiles[i - 1]) { error = "adaptive_set_tiles: the list must be strictly ascending (entry " + std::to_string(i) + ")"; return SPCBPT_ERR_INVALID_ARG; }
    }
    if (sync_all()) return SPCBPT_ERR_HIP;   // an adaptive launch may still be reading the list that is replaced
    if (n > 0) HIP_TRY(this, hipMemcpy(adaptive.list, tiles, (size_t)n * 4, hipMemcpyHostToDevice));
    adaptive.n_listed = n;
    return 0;
}

// One sample for every pixel of every listed tile: k_spcbpt_tiles into this render stream's `result` buffer, then k_film_merge_tiles as a
// link of the film-merge chain.  The eye kernel reads the counts the previous adaptive launch's merge incremented, so -- unlike an
// ordinary launch -- it waits for the chain's last link itself.  The kernel-time spans are "adaptive_eye" and "adaptive_merge".
int Context::launch_adaptive(const char* alg) {
    if (!alg || std::string(alg) != "SPCBPT_eye") { error = "launch_adaptive: \"SPCBPT_eye\" only (adaptive forms of \"pt\" and \"lt\" do not exist)"; return SPCBPT_ERR_INVALID_ARG; }
    if (kp.lens_radius > 0.0f) { error = "launch_adaptive: the list-fed eye kernel has no lens form (spcbpt_set_lens): set the lens radius to 0"; return SPCBPT_ERR_STATE; }
    if (!adaptive.active) { error = "launch_adaptive: adaptive sampling is not active (spcbpt_adaptive_begin)"; return SPCBPT_ERR_STATE; }
    if (int rc = film_ready()) return rc;
    if (!have_sampler || !have_subspace) { error = "SPCBPT_eye needs a subspace tuple and a built sampler"; return SPCBPT_ERR_STATE; }
    if (counting) { error = "launch_adaptive: not with event counters enabled (the list-fed eye kernel is a timed form: count with spcbpt_launch per frame)"; return SPCBPT_ERR_STATE; }
    if (tree_has_direction) { error = "launch_adaptive: the list-fed eye kernel caches vertex labels, which needs classifier trees without direction nodes"; return SPCBPT_ERR_STATE; }
    if (eye_sees_sky(kp)) { error = "launch_adaptive: the list-fed eye kernel does not evaluate the eye-sees-sky strategy: clear SPCBPT_ENV_EYE_SEES_SKY (spcbpt_set_environment_mode)"; return SPCBPT_ERR_STATE; }
    if (adaptive.n_listed == 0) return 0;   // nothing listed: nothing is launched, nothing changes
    int rc = begin_render(0, (int)kp.height, 1);
    if (rc) return rc;
    kp.subframe = 0;   // (unused: every tile brings its own)
    kp.counters = nullptr;
    kp.result = d_result[rk];
    sampler_tables(kp, eset);
    if (rstream != stream) HIP_TRY(this, sets[eset].sampler.wait_on(rstream));
    kp.n_tiles = (uint32_t)adaptive.n_listed;
    kp.tile_list = adaptive.list; kp.tile_samples = adaptive.samples;
    kp.work_counter = d_work_counter + rk;
    const int g = kp.scene.general != 0 ? 1 : 0;
    if (!adaptive.blocks_per_cu[g]) adaptive.blocks_per_cu[g] = spcbpt_tiles_blocks_per_cu(g != 0);
    int max_blocks = num_cus * adaptive.blocks_per_cu[g];
    const int percent = grid_percent > 0 ? grid_percent : (n_render > 1 ? 94 : 100);   // launch_render's share of the resident block slots
    if (percent < 100) max_blocks = std::max(1, max_blocks * percent / 100);
    // the spill area is indexed by the thread of the grid ACTUALLY launched: the list's tiles, capped by the resident slots
    rc = ensure_spill((size_t)spcbpt_tiles_blocks(kp, max_blocks) * (size_t)spcbpt_block_threads(), true);
    if (rc) return rc;
    if ((rc = chain_wait())) return rc;   // the counts and the film of the previous link
    HIP_TRY(this, hipMemsetAsync(d_work_counter + rk, 0, sizeof(uint32_t), rstream));
    if (!d_m2n) {   // moments on, but no merge since the last resize
        const size_t px = (size_t)kp.width * kp.height;
        HIP_TRY(this, d_m2n.reserve(px * 4));
        HIP_TRY(this, hipMemsetAsync(d_m2n, 0, px * 16, rstream));
    }
    time_begin("adaptive_eye", rstream);
    launch_spcbpt_tiles(kp, max_blocks, rstream);
    time_end();
    HIP_TRY(this, hipGetLastError());
    if ((rc = render_done(eset))) return rc;
    MergeTilesParams mp;
    memset(&mp, 0, sizeof(mp));
    mp.width = kp.width; mp.height = kp.height; mp.n_listed = (uint32_t)adaptive.n_listed;
    mp.tile_list = adaptive.list; mp.tile_samples = adaptive.samples;
    mp.result = kp.result; mp.accum = d_accum; mp.m2n = d_m2n; mp.frame = d_frame;
    time_begin("adaptive_merge", rstream);
    launch_film_merge_tiles(mp, rstream);
    time_end();
    HIP_TRY(this, hipGetLastError());
    kp.tile_list = nullptr; kp.tile_samples = nullptr;
    return chain_end();
}

int Context::read_adaptive(uint32_t* tile_samples, float* tile_error, uint32_t* tiles, int capacity, int* n) {
    if (!adaptive.active) { error = "read_adaptive: adaptive sampling is not active (spcbpt_adaptive_begin)"; return SPCBPT_ERR_STATE; }
    if (tiles && capacity < adaptive.n_listed) { error = "read_adaptive: the list holds " + std::to_string(adaptive.n_listed) + " tiles, more than `capacity`"; return SPCBPT_ERR_INVALID_ARG; }
    if (sync_all()) return SPCBPT_ERR_HIP;
    if (int rc = check_diag()) return rc;
    const size_t n_tiles = (size_t)adaptive.tiles_x * adaptive.tiles_y;
    if (tile_samples) HIP_TRY(this, hipMemcpy(tile_samples, adaptive.samples, n_tiles * 4, hipMemcpyDeviceToHost));
    if (tile_error) HIP_TRY(this, hipMemcpy(tile_error, adaptive.error, n_tiles * 4, hipMemcpyDeviceToHost));
    if (tiles && adaptive.n_listed > 0) HIP_TRY(this, hipMemcpy(tiles, adaptive.list, (size_t)adaptive.n_listed * 4, hipMemcpyDeviceToHost));
    if (n) *n = adaptive.n_listed;
    return 0;
}

}  // namespace spc

extern "C" {

int spcbpt_adaptive_begin(spcbpt_ctx* c, uint32_t frames) {
    CTX_CHECK(c);
    return c->adaptive_begin(frames);
}
int spcbpt_adaptive_end(spcbpt_ctx* c) {
    CTX_CHECK(c);
    if (!c->adaptive.active) return SPCBPT_OK;
    if (c->sync_all()) return SPCBPT_ERR_HIP;
    c->adaptive_drop();
    return SPCBPT_OK;
}
int spcbpt_adaptive_select(spcbpt_ctx* c, const spcbpt_adaptive_params* p, int* n_selected) {
    CTX_CHECK(c);
    if (!p) { c->error = "null params"; return SPCBPT_ERR_INVALID_ARG; }
    return c->adaptive_select(*p, n_selected);
}
int spcbpt_adaptive_set_tiles(spcbpt_ctx* c, const uint32_t* tiles, int n) {
    CTX_CHECK(c);
    return c->adaptive_set_tiles(tiles, n);
}
int spcbpt_launch_adaptive(spcbpt_ctx* c, const char* name) {
    CTX_CHECK(c);
    return c->launch_adaptive(name);
}
int spcbpt_read_adaptive(spcbpt_ctx* c, uint32_t* tile_samples, float* tile_error, uint32_t* tiles, int capacity, int* n) {
    CTX_CHECK(c);
    return c->read_adaptive(tile_samples, tile_error, tiles, capacity, n);
}
int spcbpt_get_adaptive_state(spcbpt_ctx* c, int* active, int* tiles_x, int* tiles_y, int* n_listed) {
    CTX_CHECK(c);
    if (active) *active = c->adaptive.active ? 1 : 0;
    if (tiles_x) *tiles_x = c->adaptive.tiles_x;
    if (tiles_y) *tiles_y = c->adaptive.tiles_y;
    if (n_listed) *n_listed = c->adaptive.n_listed;
    return SPCBPT_OK;
}

}  // extern "C"
