// Context: eye / pt launches (single, deferred, batched) and the film merges
// (part of the C ABI library: see capi_common.h for the map of its translation units)
#include "capi_common.h"
#include "kernels_merge_stats.h"

using namespace spc;

namespace spc {

static_assert(kMergeStatsMaxFrames == kMaxBatchFrames, "MergeStatsParams holds one slot per frame of a batch");

// What every launch that ends in a film merge needs before anything else ...
int Context::film_ready() {
    if (deferred.active) { error = "a deferred frame is outstanding: spcbpt_merge_deferred(ctx, keep) first"; return SPCBPT_ERR_STATE; }
    if (!d_accum) { error = "render before spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (!have_camera) { error = "render before spcbpt_set_camera"; return SPCBPT_ERR_STATE; }
    return 0;
}
// ... and, once the launch's own checks have passed: the band of rows, and the next render stream (see context.h)
int Context::begin_render(int r0, int r1, int rs) {
    if (rs < 1) rs = 1;
    if (r0 < 0 || (r0 % 8) != 0) { error = "row_begin must be a non-negative multiple of 8 (8-row bands)"; return SPCBPT_ERR_INVALID_ARG; }
    kp.row_begin = r0; kp.row_end = std::min(r1, (int)kp.height); kp.row_step = rs;
    next_render_stream();
    return 0;
}
void Context::next_render_stream() {
    rk = (rk + 1) % n_render;
    rstream = rstreams[rk];
}
// Links of the film-merge chain (the only cross-frame ordering): a link waits for the last one queued and leaves ev_merge behind for
// the next.  Film merges, feature launches and denoise passes are links (ctx_features.hip).
int Context::chain_wait() {
    if (last_merge_k >= 0 && last_merge_k != rk && rstreams[last_merge_k] != rstream) HIP_TRY(this, hipStreamWaitEvent(rstream, ev_merge[last_merge_k].ev, 0));
    return 0;
}
int Context::chain_end() {
    HIP_TRY(this, ev_merge[rk].record(rstream));
    last_merge_k = rk;
    return 0;
}
int Context::render_done(int s) {
    sets[s].render_event_of = s;
    HIP_TRY(this, sets[s].render.record(rstream));
    return 0;
}

int Context::launch_render(const char* name, bool spcbpt_alg, uint32_t frame, int r0, int r1, int rs, bool full_mis, bool defer_merge) {
    if (int rc = uniform_merge_allowed(defer_merge ? "launch_deferred" : "launch")) return rc;
    // (`!deferred.active`: film_ready's deferred-frame error keeps coming first, as it always has)
    if (!deferred.active && defer_merge && (full_mis || counting)) { error = "launch_deferred: plain \"pt\" / \"SPCBPT_eye\" launches only"; return SPCBPT_ERR_INVALID_ARG; }
    if (int rc = film_ready()) return rc;
    if (spcbpt_alg && (!have_sampler || !have_subspace)) { error = "SPCBPT_eye needs a subspace tuple and a built sampler"; return SPCBPT_ERR_STATE; }
    // the counting forms of the eye kernel know no sky strategy: a counted frame would render without it
    if (spcbpt_alg && !full_mis && kernel_variant() != 0 && eye_sees_sky(kp)) {
        error = "SPCBPT_eye: the event-counting eye kernels (counters enabled, or classifier trees with direction nodes) do not evaluate the "
                "eye-sees-sky strategy: clear SPCBPT_ENV_EYE_SEES_SKY (spcbpt_set_environment_mode) for this launch";
        return SPCBPT_ERR_STATE;
    }
    // The thin-lens camera (spcbpt_set_lens) exists as the timed single-frame eye form and as the plain "pt" form: every other form
    // refuses rather than render a pinhole image while a lens is set.
    const bool lens = kp.lens_radius > 0.0f;
    if (lens && full_mis) { error = "SPCBPT_no_rmis: not with a lens set (spcbpt_set_lens): its full-path weights assume the pinhole camera -- set the lens radius to 0 for this launch"; return SPCBPT_ERR_STATE; }
    if (lens && (spcbpt_alg ? kernel_variant() != 0 : counting)) {
        error = std::string(name) + ": the event-counting kernels (counters enabled, or classifier trees with direction nodes) have no lens form (spcbpt_set_lens): "
                "disable the counters or set the lens radius to 0 for this launch";
        return SPCBPT_ERR_STATE;
    }
    if (lens && spcbpt_alg && eye_sees_sky(kp)) {
        error = "SPCBPT_eye: the eye-sees-sky kernels have no lens form (spcbpt_set_lens): clear SPCBPT_ENV_EYE_SEES_SKY (spcbpt_set_environment_mode) or set the lens radius to 0 for this launch";
        return SPCBPT_ERR_STATE;
    }
    int rc = begin_render(r0, r1, rs);
    if (rc) return rc;
    kp.subframe = frame;
    kp.counters = counting ? d_counters.p : nullptr;
    kp.result = d_result[rk];
    if (spcbpt_alg) {
        // the sampler tables this launch reads (set `eset`) were built on `stream`
        sampler_tables(kp, eset);
        if (rstream != stream) HIP_TRY(this, sets[eset].sampler.wait_on(rstream));
    }
    rc = ensure_spill((size_t)render_thread_count(kp), true);
    if (rc) return rc;
    if (full_mis && kp.scene.env.valid) { error = "SPCBPT_no_rmis: not with an environment map (the full-path weights of cuProg.h:901-1105 know area lights only)"; return SPCBPT_ERR_STATE; }
    if (full_mis) {   // "SPCBPT_no_rmis": a plain one-lane-per-pixel launch over the same sampler tables
        time_begin(name, rstream);
        launch_spcbpt_no_rmis(kp, rstream);
        time_end();
        HIP_TRY(this, hipGetLastError());
        rc = render_done(eset);
        return rc ? rc : finish_frame();
    }
    if (spcbpt_alg) {
        kp.n_tiles = (uint32_t)render_tile_count(kp);
        kp.work_counter = d_work_counter + rk;
        HIP_TRY(this, hipMemsetAsync(d_work_counter + rk, 0, sizeof(uint32_t), rstream));
        const int generic = kernel_variant();
        if (lens && !blocks_per_cu_lens) {
            blocks_per_cu_lens = spcbpt_lens_blocks_per_cu(kp.scene.general != 0);
            if (const char* e = getenv("SPCBPT_BLOCKS_PER_CU")) { const int v = atoi(e); if (v >= 1 && v < blocks_per_cu_lens) blocks_per_cu_lens = v; }
        }
        if (!blocks_per_cu[generic]) {
            blocks_per_cu[generic] = spcbpt_blocks_per_cu(generic, false, kp.scene.general != 0, eye_sees_sky(kp));
            // developer knob (occupancy experiments): fewer resident blocks per CU than the kernel's resources allow
            if (const char* e = getenv("SPCBPT_BLOCKS_PER_CU")) { const int v = atoi(e); if (v >= 1 && v < blocks_per_cu[generic]) blocks_per_cu[generic] = v; }
            if (const char* e = getenv("SPCBPT_TILES_PER_WAVE")) tiles_per_wave = std::max(1, atoi(e));
            if (const char* e = getenv("SPCBPT_GRID_PERCENT")) grid_percent = std::max(1, std::min(100, atoi(e)));   // else adaptive
        }
    }
    time_begin(name, rstream);
    if (spcbpt_alg) {
        // Persistent grid.  With one render stream the kernel takes every resident block slot.  With several it takes 94 % of
        // them: a persistent block never yields, so a full grid leaves the next frame's light pass (and through the host's
        // wait for its vertex count, the next eye launch) nothing to run on until whole blocks have drained; with a tenth of the
        // slots free the light pass runs at once and the two eye kernels share the machine from the start.  Measured on the
        // bench scene, two streams, before the light pass ran ahead: 248 -> 259.5 Mpaths/s at 90 %, 259 at 84 %, 257.5 at 75 %; with
        // the final host loop 259.4 at 100 %, 254 at 97 %, 263.5 at 94 %, 264 at 90 % -- and the kernel by itself takes 7.95 /
        // 8.15 / 8.19 / 8.43 ms at those shares, so 94 % it is.  A policy that looks whether the previous eye kernel is still running does
        // not work: by the time the host has the vertex count it waited for, that kernel has drained.
        // SPCBPT_GRID_PERCENT fixes the share; SPCBPT_TILES_PER_WAVE bounds the waves by the tile count (experiments).
        const int generic = kernel_variant();
        int max_blocks = num_cus * (lens ? blocks_per_cu_lens : blocks_per_cu[generic]);
        if (tiles_per_wave > 1) max_blocks = std::max(1, std::min(max_blocks, (int)(kp.n_tiles / (uint32_t)(4 * tiles_per_wave))));
        const int percent = grid_percent > 0 ? grid_percent : (n_render > 1 ? 94 : 100);
        if (percent < 100) max_blocks = std::max(1, max_blocks * percent / 100);
        if (lens) launch_spcbpt_lens(kp, max_blocks, rstream);   // (its grid is at most the tile range's: the spill area above covers it)
        else launch_spcbpt(kp, generic, max_blocks, rstream);
    }
    else if (lens) launch_pt_lens(kp, rstream);
    else launch_pt(kp, counting, rstream);
    time_end();
    HIP_TRY(this, hipGetLastError());
    if (spcbpt_alg && (rc = render_done(eset))) return rc;
    if (defer_merge) {
        deferred.active = true; deferred.rk = rk; deferred.subframe = kp.subframe; deferred.result = kp.result;
        deferred.row_begin = kp.row_begin; deferred.row_end = kp.row_end; deferred.row_step = kp.row_step;
        return 0;
    }
    return finish_frame();
}

// The film merge of the deferred frame, now (keep) or never.  Dropping costs nothing but the kernel time already spent: the
// render kernel wrote its own `result` buffer only.
int Context::merge_deferred(bool keep) {
    if (!deferred.active) { error = "merge_deferred: no deferred frame"; return SPCBPT_ERR_STATE; }
    deferred.active = false;
    if (!keep) return 0;
    rk = deferred.rk;
    rstream = rstreams[rk];
    kp.subframe = deferred.subframe; kp.result = deferred.result;
    kp.row_begin = deferred.row_begin; kp.row_end = deferred.row_end; kp.row_step = deferred.row_step;
    return finish_frame();
}
// Host wait for the last film merge only (the frame to be displayed), not for work queued behind it (the next frame's light
// pass, sampler build and speculative eye launch).
int Context::sync_film() {
    if (last_merge_k >= 0 && ev_merge[last_merge_k].set) HIP_TRY(this, hipEventSynchronize(ev_merge[last_merge_k].ev));
    return check_diag();
}

int Context::launch_eye_batch(int n, const uint32_t* subframes, int r0, int r1, int rs) { return batch_render("launch_eye_batch", false, n, subframes, r0, r1, rs); }
int Context::launch_eye_batch_film(int n, const uint32_t* subframes, int r0, int r1, int rs) { return batch_render("launch_eye_batch_film", true, n, subframes, r0, r1, rs); }

// `film`: the merge keeps the second moment and fills the buckets, whichever are on (k_film_merge_batch_stats); without it the launch
// refuses while either is on, as it always has
int Context::batch_render(const char* name, bool film, int n, const uint32_t* subframes, int r0, int r1, int rs) {
    const std::string who(name);
    int rc = uniform_merge_allowed(name);
    if (rc) return rc;
    if ((rc = film_ready())) return rc;
    if (!film && film_moments) {
        error = "launch_eye_batch: not with film moments enabled (spcbpt_set_film_moments): the batched merge takes up to 32 frames per pixel in one "
                "pass and keeps no second moment (use spcbpt_launch per frame, or spcbpt_launch_eye_batch_film)";
        return SPCBPT_ERR_STATE;
    }
    if (!film && film_buckets) {
        error = "launch_eye_batch: not with the film's buckets on (spcbpt_set_film_buckets): the batched merge takes up to 32 frames per pixel in one "
                "pass and fills no buckets (use spcbpt_launch per frame, or spcbpt_launch_eye_batch_film)";
        return SPCBPT_ERR_STATE;
    }
    if (kp.lens_radius > 0.0f) { error = who + ": the batched eye kernel has no lens form (spcbpt_set_lens): use spcbpt_launch per frame, or set the lens radius to 0"; return SPCBPT_ERR_STATE; }
    if (!have_subspace) { error = "SPCBPT_eye needs a subspace tuple and a built sampler"; return SPCBPT_ERR_STATE; }
    if (n < 1 || n > kMaxBatchFrames || !subframes) { error = who + ": 1..32 frames"; return SPCBPT_ERR_INVALID_ARG; }
    if (n > (int)built_sets.size()) { error = who + ": fewer samplers have been built (and are still intact) than frames were asked for"; return SPCBPT_ERR_STATE; }
    // (SPCBPT_EYE_BATCH at spcbpt_create only sizes the ring of buffer sets so that batches, light passes ahead and builds do not
    // wait for each other; correctness rests on the per-set events and on `built_sets` naming intact samplers)
    if (counting) { error = who + ": not with event counters enabled (count with spcbpt_launch per frame)"; return SPCBPT_ERR_STATE; }
    if (tree_has_direction) { error = who + ": the batched kernel caches vertex labels, which needs classifier trees without direction nodes (use spcbpt_launch per frame)"; return SPCBPT_ERR_STATE; }
    if (kp.width >= 65536u || kp.height >= 65536u) { error = who + ": image too large"; return SPCBPT_ERR_INVALID_ARG; }
    if ((rc = begin_render(r0, r1, rs))) return rc;
    kp.counters = nullptr;
    const size_t px = (size_t)kp.width * kp.height;
    if (!h_frames) HIP_TRY(this, hipHostMalloc(reinterpret_cast<void**>(&h_frames), sizeof(FrameDesc) * kMaxRender * kDescRing * kMaxBatchFrames));
    HIP_TRY(this, d_frames[rk].reserve(kMaxBatchFrames));
    // the descriptors travel through a small ring of pinned slots: the host must not wait for the previous batch of this stream
    // (it would stop launching the light passes of the batches after it), only for the upload that used this slot 4 batches ago
    const int gen = desc_gen[rk]++ % kDescRing;
    FrameDesc* hf = h_frames + ((size_t)rk * kDescRing + gen) * kMaxBatchFrames;
    if (ev_desc[rk][gen]) HIP_TRY(this, hipEventSynchronize(ev_desc[rk][gen]));
    else HIP_TRY(this, hipEventCreateWithFlags(&ev_desc[rk][gen], hipEventDisableTiming));
    int batch[kMaxBatchFrames];
    for (int k = 0; k < n; k++) {
        const int e = batch[k] = built_sets[built_sets.size() - (size_t)n + (size_t)k];   // oldest of the last n first
        HIP_TRY(this, d_result_b[rk][k].reserve(px * 4));
        sampler_tables(hf[k], e);
        hf[k].result = d_result_b[rk][k]; hf[k].subframe = subframes[k];
        if (rstream != stream) HIP_TRY(this, sets[e].sampler.wait_on(rstream));
    }
    HIP_TRY(this, hipMemcpyAsync(d_frames[rk], hf, sizeof(FrameDesc) * (size_t)n, hipMemcpyHostToDevice, rstream));
    HIP_TRY(this, hipEventRecord(ev_desc[rk][gen], rstream));
    kp.n_tiles = (uint32_t)render_tile_count(kp);
    kp.frames = d_frames[rk]; kp.n_frames = (uint32_t)n;
    kp.work_counter = d_work_counter + rk;
    kp.result = nullptr; kp.subframe = subframes[0];
    HIP_TRY(this, hipMemsetAsync(d_work_counter + rk, 0, sizeof(uint32_t), rstream));
    if (!blocks_per_cu_batch) blocks_per_cu_batch = spcbpt_blocks_per_cu(0, true, kp.scene.general != 0, eye_sees_sky(kp));
    int max_blocks = num_cus * blocks_per_cu_batch;
    // a batch kernel runs for tens of milliseconds: the light passes of the batches after it need block slots meanwhile -- few,
    // since they run as a thin grid (launch_light_batch): 97 % (64 steps on one GPU: 5.76 ms per step at 94 %, 5.69 at 97, 5.67 at 100;
    // a rank's share of a sharded frame is indifferent: 0.81-0.82 ms per rank-frame at N = 8 with all three)
    const int percent = grid_percent > 0 ? grid_percent : 97;
    if (percent < 100) max_blocks = std::max(1, max_blocks * percent / 100);
    // the spill area is indexed by the thread of the grid ACTUALLY launched: n frames' tiles, capped by the resident slots
    // (sizing it for one frame's tiles let the blocks beyond one frame's share write past its end whenever that share was below max_blocks)
    rc = ensure_spill((size_t)spcbpt_batch_blocks(kp, max_blocks) * (size_t)spcbpt_block_threads(), true);
    if (rc) return rc;
    time_begin("spcbpt_render", rstream);
    launch_spcbpt_batch(kp, max_blocks, rstream);
    time_end();
    HIP_TRY(this, hipGetLastError());
    eset = batch[n - 1];
    HIP_TRY(this, sets[eset].render.record(rstream));   // ONE event for the sets of the batch (context.h: CacheSet::render_event_of)
    for (int k = 0; k < n; k++) { sets[batch[k]].render_event_of = eset; sets[batch[k]].render.set = true; }
    // the frames' merges, in frame order, after the previous launch's merge
    if ((rc = chain_wait())) return rc;
    if (film && (film_moments || film_buckets)) {
        // ... as one pass that also does, per frame, what moments_step and buckets_step do in front of a single merge
        // (kernels_merge_stats.hip: k_film_merge_batch_stats); the planes as those steps set them up
        if (film_moments && !d_m2n) {
            HIP_TRY(this, d_m2n.reserve(px * 4));
            HIP_TRY(this, hipMemsetAsync(d_m2n, 0, px * 16, rstream));
        }
        if (film_buckets && (rc = ensure_buckets(rstream))) return rc;
        MergeStatsParams mp;
        memset(&mp, 0, sizeof(mp));
        mp.width = kp.width; mp.height = kp.height;
        mp.row_begin = kp.row_begin; mp.row_end = kp.row_end; mp.row_step = kp.row_step;
        mp.frames = n; mp.buckets = film_buckets;
        mp.accum = d_accum; mp.frame = kp.frame;
        mp.m2n = film_moments ? d_m2n.p : nullptr; mp.planes = film_buckets ? d_buckets.p : nullptr;
        for (int k = 0; k < n; k++) { mp.result[k] = d_result_b[rk][k]; mp.subframe[k] = subframes[k]; }
        kp.subframe = subframes[n - 1];
        kp.result = d_result_b[rk][0];
        time_begin("film_merge_stats", rstream);
        launch_film_merge_batch_stats(mp, rstream);
        time_end();
        HIP_TRY(this, hipGetLastError());
    }
    else {   // ... as one pass over the pixels (kernels.hip: k_film_merge_batch -- the operations of n merges, per pixel in frame order)
        MergeBatch mb = {};
        for (int k = 0; k < n; k++) { mb.result[k] = d_result_b[rk][k]; mb.subframe[k] = subframes[k]; }
        kp.subframe = subframes[n - 1];
        kp.result = d_result_b[rk][0];
        launch_film_merge_batch(kp, mb, n, rstream);
        HIP_TRY(this, hipGetLastError());
    }
    kp.frames = nullptr; kp.n_frames = 0;
    return chain_end();
}

// merge this launch's `result` into accum / frame, after the previous launch's merge (the only cross-frame ordering); with film moments
// enabled the second moment of the same pixels is updated first, from the mean the merge is about to replace (ctx_moments.hip)
int Context::finish_frame() {
    if (int rc = chain_wait()) return rc;
    if (film_moments) { if (int rc = moments_step()) return rc; }
    if (film_buckets) { if (int rc = buckets_step()) return rc; }   // ... and with the bucket film on, the sample's bucket (ctx_buckets.hip)
    time_begin("film_merge", rstream);   // (the kernel-time span adaptive sampling's "adaptive_merge" is compared with)
    launch_film_merge(kp, rstream);
    time_end();
    HIP_TRY(this, hipGetLastError());
    return chain_end();
}

}  // namespace spc
