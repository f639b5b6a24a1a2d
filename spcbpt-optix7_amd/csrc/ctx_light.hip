// Context: light passes (single and batched) and the device sampler build (MyThrustOp::LVC_Process, cuda_thrust/device_thrust.cu:241-332)
// (part of the C ABI library: see capi_common.h for the map of its translation units)
#include "capi_common.h"

using namespace spc;

namespace spc {

// `ls` is about to queue a light pass that rewrites set s: it waits for the last eye kernel that read the set (the sets of one batched
// eye launch share one event: `waited_for` names the one already waited for), and -- unless `ls` is `stream` itself -- for a sampler
// build or an import copy of the set's previous contents that may still be queued on `stream` (a set that was built or imported but
// never rendered carries no fresh render event), and for a gathered import of them (exchange stream).
int Context::begin_rewrite(hipStream_t ls, int s, int& waited_for) {
    CacheSet& S = sets[s];
    if (S.render.set && S.render_event_of != waited_for) {
        HIP_TRY(this, hipStreamWaitEvent(ls, sets[S.render_event_of].render.ev, 0));
        waited_for = S.render_event_of;
    }
    if (ls != stream) HIP_TRY(this, S.on_stream.wait_on(ls));
    HIP_TRY(this, S.exch.wait_on(ls));
    S.bound = -1;
    return 0;
}
static void drop(std::deque<int>& q, int s) {
    for (auto it = q.begin(); it != q.end();) it = (*it == s) ? q.erase(it) : it + 1;
}
void Context::set_rewritten(int s) {
    drop(built_sets, s);                     // its sampler is gone
    if (keys_set == s) keys_ready = false;   // lane 0's keys no longer describe the set
}
int Context::pass_traced(hipStream_t ls, int s, int lane) {
    CacheSet& S = sets[s];
    HIP_TRY(this, S.light.record(ls));
    S.count_host = -1;
    S.light_counts_valid = true;
    S.light_lane = lane;
    set_rewritten(s);
    drop(pending, s);   // a set that comes round again unbuilt
    pending.push_back(s);
    return 0;
}
int Context::sampler_built(int s) {
    eset = s;
    HIP_TRY(this, sets[s].sampler.record(stream));
    HIP_TRY(this, sets[s].on_stream.record(stream));
    drop(built_sets, s);
    built_sets.push_back(s);
    while ((int)built_sets.size() > kMaxBatchFrames) built_sets.pop_front();
    if (!pending.empty() && pending.front() == s) pending.pop_front();
    return 0;
}
void Context::contents_imported(int s, int count_host, int bound) {
    CacheSet& S = sets[s];
    S.count_host = count_host;
    S.bound = bound;
    S.light_counts_valid = false;
    S.light_lane = 0;   // from here on the set's contents are ordered on `stream` (or by its `exch` event)
    set_rewritten(s);   // a sampler built from the old contents is gone
    if (s == lset) lvc_count = count_host;
    have_sampler = false;
}

int Context::light_pass_params(uint32_t frame, int n_frames, LightVertex* scratch, int* core_counts, bool count_events, DevBuf<uint32_t>& spill, int grid_cap) {
    kp.num_core = lt.num_core; kp.core_padding = lt.core_padding; kp.m_per_core = lt.m_per_core;
    kp.core_begin = lt.core_begin; kp.core_count = lt.core_count; kp.launch_frame = frame;
    kp.n_lframes = n_frames;   // 0: one pass (a batched launch that failed half-way must not leave its mode behind)
    kp.lt_decorrelate = lt.decorrelate_bsdf_stream;
    kp.lvc_scratch = scratch; kp.core_counts = core_counts;
    kp.counters = count_events ? d_counters.p : nullptr;
    if (light_blocks < 0) { const char* lb = getenv("SPCBPT_LIGHT_BLOCKS"); light_blocks = lb ? std::max(1, atoi(lb)) : std::max(1, num_cus); }
    // traversal-stack spill area: TravStack indexes it by blockIdx.x * 256 + threadIdx.x of the grid launched (launch_light_trace)
    const size_t threads = n_frames ? (size_t)light_trace_blocks(kp, grid_cap) * 256 : ((size_t)lt.core_count + 255) / 256 * 256;
    const int entries = spill_entries_needed();
    kp.spill_entries = entries;
    if (entries == 0) { kp.spill = nullptr; return 0; }
    if (n_frames && threads * (size_t)entries > spill.cap && sync_all()) return SPCBPT_ERR_HIP;   // (a single pass leaves the wait to hipFree)
    HIP_TRY(this, spill.reserve(threads * (size_t)entries));
    kp.spill = spill;
    return 0;
}

// "light trace": k_light_trace into the padded scratch, then compaction into the deterministic (core, slot) order
int Context::launch_light(uint32_t frame) {
    if (!have_subspace) { error = "light trace needs a subspace tuple (spcbpt_set_subspace)"; return SPCBPT_ERR_STATE; }
    if (!lanes[0].scratch) {
        spcbpt_light_trace_params d = {100000, 52, 1, 0, 0, 1};
        int rc = set_light_trace(d);
        if (rc) return rc;
    }
    if (lvc_probe_needed) { int rcp = probe_lvc_capacity(); if (rcp) return rcp; }
    // lane: passes running ahead alternate between the light stream and a second one (context.h); everything else uses lane 0
    int lane = 0;
    if (light_ahead && !counting && getenv("SPCBPT_LIGHT_LANES") == nullptr) { light_toggle ^= 1; lane = light_toggle; }
    if (lane) { int rcb = ensure_lane_b(); if (rcb) return rcb; }
    LightLane& L = lanes[lane];
    const hipStream_t ls = L.stream;
    int rc = light_pass_params(frame, 0, L.scratch, L.core_counts, counting, L.spill, 0);
    if (rc) return rc;
    // write the set the eye pass is NOT reading; it was last read by the render launch before the previous one
    lset = (lset + 1) % n_sets;
    CacheSet& S = sets[lset];
    int waited_for = -1;
    rc = begin_rewrite(ls, lset, waited_for);
    if (rc) return rc;
    HIP_TRY(this, hipMemsetAsync(L.core_counts, 0, ((size_t)lt.core_count + 1) * sizeof(int), ls));
    HIP_TRY(this, hipMemsetAsync(S.counts, 0, 2 * sizeof(int), ls));
    kp.path_counter = S.counts + 1;
    // persistent grid of the light pass: at most light_blocks blocks pull cores from a queue (kernels.hip)
    kp.work_counter = L.work_counter;
    HIP_TRY(this, hipMemsetAsync(kp.work_counter, 0, sizeof(uint32_t), ls));
    // Thin or wide (round 6).  One block per CU is right for a pass that runs BESIDE eye kernels (light-ahead mode: few long-lived blocks
    // take least from them).  In the reference's loop form -- light pass, build, eye launch, sync, strictly in turn
    // (optixPathTracer.cpp:791-822) -- nothing else is on the GPU while the pass runs, and one wave per SIMD leaves it a chain of
    // dependent fetches: there the pass gets a lane per core (100 000 paths: 391 blocks; four per CU at most), SPCBPT_LIGHT_BLOCKS_WIDE.
    if (light_blocks_wide < 0) { const char* lb = getenv("SPCBPT_LIGHT_BLOCKS_WIDE"); light_blocks_wide = lb ? std::max(1, atoi(lb)) : std::max(1, 4 * num_cus); }
    const int light_grid = (!light_ahead && lane == 0) ? std::max(light_blocks, light_blocks_wide) : light_blocks;
    time_begin("light_trace", ls);
    launch_light_trace(kp, kernel_variant(), light_grid, ls);   // direction trees: the generic instantiation (no label caching)
    time_end();
    HIP_TRY(this, hipGetLastError());
    // compaction: exclusive scan of per-core counts (+1 sentinel gives the total) -> offsets
    time_begin("lvc_compact", ls);
    size_t tb = 0;
    HIP_TRY(this, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, L.core_counts.p, L.core_offsets.p, lt.core_count + 1, ls));
    HIP_TRY(this, L.temp.reserve(tb));
    HIP_TRY(this, hipcub::DeviceScan::ExclusiveSum(L.temp.p, tb, L.core_counts.p, L.core_offsets.p, lt.core_count + 1, ls));
    HIP_TRY(this, hipMemcpyAsync(S.counts, L.core_offsets + lt.core_count, sizeof(int), hipMemcpyDeviceToDevice, ls));
    launch_lvc_compact(L.scratch, L.core_counts, L.core_offsets, lt.core_count, lt.core_padding, S.lvc, L.keys, L.vals, L.weights,
                       S.counts, (int)std::min<size_t>(lvc_capacity, 0x7fffffff), d_diag + 2, ls);
    time_end();
    HIP_TRY(this, hipGetLastError());
    lvc_count = -1;  // known on the device only until the next host read
    // A new light pass means "build before you render", as in the reference's loop -- also with passes running ahead: a host loop
    // that launches a pass and forgets the build gets SPCBPT_ERR_STATE from its next eye launch, not last frame's sampler.  The
    // tables of set `eset` are in fact still intact while later passes fill OTHER sets of the ring; a host that means to render
    // from them once more (csrc/viewer.cpp: a speculative frame dropped and traced again) says so with spcbpt_reuse_sampler.
    have_sampler = false;
    // (vertex_count, path_count) to pinned host memory, inside the event: the sampler build reads them after waiting for
    // THIS pass only, not for whatever else has been queued on the stream since
    HIP_TRY(this, hipMemcpyAsync(h_light_counts + 2 * lset, S.counts, 2 * sizeof(int), hipMemcpyDeviceToHost, ls));
    if (!light_ahead) pending.clear();   // default: a sampler build always takes the latest light pass
    rc = pass_traced(ls, lset, lane);
    if (rc) return rc;
    if (lane == 0) { keys_ready = true; keys_set = lset; }   // (the other lane's keys describe nothing the build reads)
    return 0;
}

// Batched light pass: see context.h.  Sets lset+1 .. lset+n receive the passes of launch frames first_frame .. first_frame+n-1 and
// queue up in `pending` like n calls of launch_light; every one of them is bit-identical to the pass launch_light would have traced
// (same seeds per core, same (core, slot) order after compaction).
int Context::launch_light_batch(uint32_t first_frame, int n) {
    if (!have_subspace) { error = "light trace needs a subspace tuple (spcbpt_set_subspace)"; return SPCBPT_ERR_STATE; }
    if (n < 1 || n > kMaxBatchFrames || n > n_sets - 2) { error = "launch_light_batch: 1 .. min(32, sets - 2) frames per batch"; return SPCBPT_ERR_INVALID_ARG; }
    if (!light_ahead) { error = "launch_light_batch: the passes queue up for build_sampler -- enable spcbpt_set_light_ahead first"; return SPCBPT_ERR_STATE; }
    if (!lanes[0].scratch) {
        spcbpt_light_trace_params d = {100000, 52, 1, 0, 0, 1};
        int rc = set_light_trace(d);
        if (rc) return rc;
    }
    if (lvc_probe_needed) { int rcp = probe_lvc_capacity(); if (rcp) return rcp; }
    int rc = ensure_lane_b();
    if (rc) return rc;
    const hipStream_t ls = lanes[1].stream;
    const size_t slots = (size_t)lt.core_count * lt.core_padding, cstride = (size_t)lt.core_count + 1;
    if ((size_t)n * slots > lb_scratch.cap || (size_t)n * cstride > lb_core_counts.cap) {
        if (sync_all()) return SPCBPT_ERR_HIP;
        HIP_TRY(this, lb_scratch.reserve((size_t)n * slots));
        HIP_TRY(this, lb_core_counts.reserve((size_t)n * cstride)); HIP_TRY(this, lb_core_offsets.reserve((size_t)n * cstride));
        HIP_TRY(this, lb_path_counts.reserve((size_t)kMaxBatchFrames));
    }
    // a THIN grid: the batch runs beside the eye kernels of the frames before it and only has to be done before they are; few
    // long-lived blocks take less from them than many (bench scene, one GPU, 20 / 64 steps, ms per step: 16 blocks 5.71 / 5.67,
    // 24: 5.73 / 5.66, 32: 5.74 / 5.68, 48: 5.85 / 5.71, 64: 5.94 / 5.76 -- the 20-frame batch then takes 76 ms beside an eye launch
    // of 110).  SPCBPT_LIGHT_BATCH_BLOCKS fixes the number; by default it goes ...
    if (light_batch_blocks < 0) { const char* lb = getenv("SPCBPT_LIGHT_BATCH_BLOCKS"); light_batch_blocks = lb ? std::max(1, atoi(lb)) : 0; }
    int grid_cap = light_batch_blocks;
    if (grid_cap == 0) {
        // ... in proportion to the light paths per pixel of this context's share of the frame (kp.row_step: the band step of the last
        // eye launch), so that the batch stays shorter than the eye launch it runs beside: 640 blocks per (path / pixel), i.e. 32 for
        // 100 000 paths against 1920 x 1080 pixels -- or against an eighth of both
        const double px = std::max(1.0, (double)kp.width * kp.height / std::max(1, (int)kp.row_step));
        const double ratio = (double)lt.core_count * std::max(1, lt.m_per_core) / px;
        // (a rank's share of a sharded frame wants more lanes for the same ratio: its eye launches are short, and the chain of a
        // batch -- passes, then one exchange and build per frame -- has to fit under them: N = 8 simulation 0.80-0.81 ms per
        // rank-frame with 48 blocks, 0.83-0.87 with 20)
        // (round 4: 400 -> 480 blocks per (path / pixel).  With the eye kernel 13 % faster the 20 blocks of 400 finished a 20-frame batch in
        // 75 ms beside an eye launch of 83 -- and 16 blocks, too few, cost 10 %: the batch became the critical path.  24 keep a fifth in hand
        // at no measurable cost: 20 / 24 / 28 / 32 blocks 4.176 / 4.204 / 4.181 / 4.231 ms per step)
        // (round 5: 480 -> 640, i.e. 32.  The eye kernel is another 8 % faster and runs its traversal pass at a raised issue priority, under
        // which the light pass that shares its CUs is slower: with 24 blocks the batch for the NEXT eye launch took 101-113 ms beside an eye
        // launch of 116 (tools/timeline_long.sh), so that its sampler build -- 1.3 ms -- ran in the gap between two eye kernels instead of
        // under the first.  Steady-state ms per step, 24 / 32 / 40 / 48 / 64 blocks: 3.706 / 3.661 / 3.70-3.77 / 3.75 / 3.87)
        // (round 6, advisor: 640 x 0.048225 = 30.9 -> ceil gave 31, a grid no sweep had covered; the product is now rounded up to a
        // multiple of 8 blocks -- one per XCD -- which IS the swept 32 on the bench scene)
        grid_cap = (int)std::max(kp.row_step > 1 ? 48.0 : 16.0, std::min(256.0, 8.0 * std::ceil(80.0 * ratio)));
    }
    // (cores that trace many paths one after the other -- the reference's geometry -- are long jobs: never two of them per lane)
    if (lt.m_per_core >= 8) grid_cap = std::max(grid_cap, (int)(((long long)n * lt.core_count + 255) / 256));
    rc = light_pass_params(first_frame, n, lb_scratch, lb_core_counts, counting, lb_spill, grid_cap);
    if (rc) return rc;
    kp.path_counter = lb_path_counts;
    CompactBatch dst = {};
    int batch[kMaxBatchFrames];
    int waited_for = -1;
    for (int k = 0; k < n; k++) {   // what launch_light waits for before it rewrites a set, for every set of the batch
        const int s = batch[k] = (lset + 1 + k) % n_sets;
        rc = begin_rewrite(ls, s, waited_for);
        if (rc) return rc;
        dst.lvc[k] = sets[s].lvc; dst.counts[k] = sets[s].counts;
    }
    HIP_TRY(this, hipMemsetAsync(lb_core_counts, 0, (size_t)n * cstride * sizeof(int), ls));
    HIP_TRY(this, hipMemsetAsync(lb_path_counts, 0, kMaxBatchFrames * sizeof(int), ls));
    kp.work_counter = lanes[1].work_counter;   // the second lane's queue head
    HIP_TRY(this, hipMemsetAsync(kp.work_counter, 0, sizeof(uint32_t), ls));
    time_begin("light_trace", ls);
    launch_light_trace(kp, kernel_variant(), grid_cap, ls);
    time_end();
    kp.n_lframes = 0;
    HIP_TRY(this, hipGetLastError());
    time_begin("lvc_compact", ls);
    size_t tb = 0;
    const int items = (int)((size_t)n * cstride);
    DevBuf<unsigned char>& temp = lanes[1].temp;
    HIP_TRY(this, hipcub::DeviceScan::ExclusiveSum(nullptr, tb, lb_core_counts.p, lb_core_offsets.p, items, ls));
    if (tb > temp.cap && sync_all()) return SPCBPT_ERR_HIP;
    HIP_TRY(this, temp.reserve(tb));
    HIP_TRY(this, hipcub::DeviceScan::ExclusiveSum(temp.p, tb, lb_core_counts.p, lb_core_offsets.p, items, ls));
    launch_lvc_compact_batch(lb_scratch, lb_core_counts, lb_core_offsets, lb_path_counts, lt.core_count, lt.core_padding, n, dst,
                             (int)std::min<size_t>(lvc_capacity, 0x7fffffff), d_diag + 2, ls);
    time_end();
    HIP_TRY(this, hipGetLastError());
    // (vertex_count, path_count) of the sets to pinned host memory: the sets are consecutive modulo n_sets -> at most two ranges
    {
        const int s0 = batch[0], first = std::min(n, n_sets - s0);
        HIP_TRY(this, hipMemcpyAsync(h_light_counts + 2 * s0, d_set_counts_all + 2 * s0, (size_t)first * 2 * sizeof(int), hipMemcpyDeviceToHost, ls));
        if (first < n) HIP_TRY(this, hipMemcpyAsync(h_light_counts, d_set_counts_all, (size_t)(n - first) * 2 * sizeof(int), hipMemcpyDeviceToHost, ls));
    }
    for (int k = 0; k < n; k++) { rc = pass_traced(ls, batch[k], 1); if (rc) return rc; }
    lset = batch[n - 1];
    lvc_count = -1;
    have_sampler = false;
    return 0;
}

int Context::fetch_counts_of(int set) {
    int h[2] = {0, 0};
    if (sets[set].light_counts_valid && sets[set].light_lane != 0) HIP_TRY(this, hipEventSynchronize(sets[set].light.ev));   // traced on the second lane: `stream` does not order it
    HIP_TRY(this, hipMemcpyAsync(h, sets[set].counts, sizeof(h), hipMemcpyDeviceToHost, stream));
    HIP_TRY(this, hipStreamSynchronize(stream));
    lvc_count = h[0];
    path_count = h[1];
    return 0;
}
int Context::fetch_counts() { return fetch_counts_of(lset); }

// LVC_Process on the device, for the oldest light pass (or imported cache) that has no sampler yet
int Context::build_sampler() {
    if (!sets[lset].lvc) { error = "build_sampler: no light-vertex cache (run \"light trace\" or spcbpt_lvc_import first)"; return SPCBPT_ERR_STATE; }
    const int bset = build_set();
    CacheSet& S = sets[bset];
    LightLane& L = lanes[0];   // the build's keys, values, weights and temp area are lane 0's
    int rc = 0;
    if (S.light_lane != 0 && S.light_counts_valid) HIP_TRY(this, S.light.wait_on(stream));   // traced on the second lane
    // the radix sort needs its item count on the host: an import told it, or the light pass left it in pinned memory (wait for
    // that pass's event), or -- a cache written some other way -- one 8-byte readback
    const bool dev_count = S.bound >= 0;   // gathered import: totals on the device, build over the upper bound
    if (dev_count) HIP_TRY(this, S.exch.wait_on(stream));
    bool count_known = S.count_host >= 0 || dev_count;
    // the counting build takes its item count on the device: a light pass's (vertex_count, path_count) need not reach the host first --
    // the reference-shaped loop (light pass -> build -> eye launch, one sync per frame) then runs without a host wait in the middle
    const bool lazy = counting_build && !count_known && S.light_counts_valid;
    if (dev_count) { lvc_count = S.bound; path_count = -1; }
    else if (count_known) lvc_count = S.count_host;
    else if (lazy) { lvc_count = (int)std::min<size_t>(lvc_capacity, 0x7fffffff); path_count = -1; count_known = true; }
    else if (S.light_counts_valid) {
        HIP_TRY(this, hipEventSynchronize(S.light.ev));
        lvc_count = h_light_counts[2 * bset]; path_count = h_light_counts[2 * bset + 1];
        count_known = true;
    } else rc = fetch_counts_of(bset);
    if (rc) return rc;
    const int n = lvc_count;
    time_begin("sampler_build");
    if (counting_build) {
        // one stable counting sort over the 10-bit subspace ids: four launches (kernels.hip).  The path count is taken on the way
        // unless the light pass (or the gathered import) has left it in the set already.
        HIP_TRY(this, d_hist.reserve(sampler_build_hist_ints()));
        const bool count_paths = !dev_count && !lazy && !(keys_ready && keys_set == bset);   // (a light pass has left the path count in its set)
        if (count_paths) HIP_TRY(this, hipMemsetAsync(S.counts + 1, 0, sizeof(int), stream));
        launch_sampler_build(S.lvc, n, (dev_count || lazy) ? S.counts : nullptr, L.keys, L.weights, d_hist, count_paths ? S.counts + 1 : nullptr,
                             S.subspace, S.jump, d_wsorted, S.cmfs, S.lvc_sorted, S.guide, stream);
        keys_ready = false;
    } else {
    if (dev_count) {
        launch_fill_keys_devcount(S.lvc, n, L.keys, L.vals, L.weights, S.counts, stream);
    } else if (!(keys_ready && keys_set == bset)) {
        HIP_TRY(this, hipMemsetAsync(S.counts + 1, 0, sizeof(int), stream));
        launch_fill_keys(S.lvc, n, L.keys, L.vals, L.weights, S.counts, stream);
    }
    keys_ready = false;   // the sort below consumes the keys
    HIP_TRY(this, hipMemsetAsync(S.subspace, 0, SPCBPT_NUM_SUBSPACE * sizeof(DSubspace), stream));
    if (n > 0) {
        size_t tb = 0, tb2 = 0;
        HIP_TRY(this, hipcub::DeviceRadixSort::SortPairs(nullptr, tb, L.keys.p, d_keys2.p, L.vals.p, S.jump.p, n, 0, 10, stream));
        HIP_TRY(this, hipcub::DeviceScan::InclusiveSum(nullptr, tb2, d_wsorted.p, d_prefix.p, n, stream));
        rc = ensure_temp(std::max(tb, tb2));
        if (rc) return rc;
        HIP_TRY(this, hipcub::DeviceRadixSort::SortPairs(L.temp.p, tb, L.keys.p, d_keys2.p, L.vals.p, S.jump.p, n, 0, 10, stream));
        launch_subspace_ranges(d_keys2, S.counts, S.subspace, n, stream);
        launch_gather_weights(L.weights, S.jump, S.counts, d_wsorted, n, stream);
        HIP_TRY(this, hipcub::DeviceScan::InclusiveSum(L.temp.p, tb2, d_wsorted.p, d_prefix.p, n, stream));
        launch_cmf(d_prefix, d_keys2, S.counts, S.subspace, S.cmfs, n, stream);
        launch_lvc_sorted_copy(S.lvc, S.jump, S.counts, S.lvc_sorted, n, stream);
        launch_sampler_guide(S.subspace, S.cmfs, S.guide, stream);
    }
    }
    time_end();
    HIP_TRY(this, hipGetLastError());
    // the host copy of (vertex_count, path_count): a second readback, skipped when the count came with an import (a sharded
    // job must not wait for the light stream here -- the next frame's light pass is already queued on it)
    if (!count_known && fetch_counts_of(bset)) return SPCBPT_ERR_HIP;
    rc = sampler_built(bset);
    if (rc) return rc;
    have_sampler = true;
    if (dev_count || lazy) lvc_count = -1;   // the host does not know it (fetch_counts brings it when somebody asks)
    return 0;
}

void Context::free_batch_build_scratch() {
    sbb_keys.release(); sbb_weights.release(); sbb_wsorted.release(); sbb_hist.release();
    sbb_frames = 0; sbb_capacity = 0;
}
size_t Context::sbb_debug_limit() const {
    const char* e = getenv("SPCBPT_DEBUG_BATCH_SCRATCH_LIMIT");
    return e ? (size_t)strtoull(e, nullptr, 10) : ~(size_t)0;
}

// LVC_Process for the n OLDEST light passes that have no sampler yet, as ONE set of four launches (kernels.hip: SamplerBuildBatch).
// The tables are those of n build_sampler calls -- the same kernels with the frame in blockIdx.y -- and the sets end up in the same
// state; what goes is n - 1 times the four dependent launches (0.12 ms per build: 2.4 ms in front of a 20-frame eye launch that
// cannot start before the last of them).  Gathered imports (totals on the device) are built over their upper bound, as build_sampler
// does.  Falls back to n single builds for the radix-sort form and for a cache whose counts the host would have to read back.
int Context::build_sampler_batch(int n) {
    if (n < 1 || n > kMaxBatchFrames) { error = "build_sampler_batch: 1 .. 32 builds per call"; return SPCBPT_ERR_INVALID_ARG; }
    bool plain = counting_build && n > 1 && sets[lset].lvc && (int)pending.size() >= n;
    for (int k = 0; plain && k < n; k++) {
        const int b = pending[(size_t)k];
        if (sets[b].bound < 0 && !(sets[b].count_host >= 0 || sets[b].light_counts_valid)) plain = false;   // counts the host would have to read back
    }
    if (!plain) {
        for (int k = 0; k < n; k++) { const int rc = build_sampler(); if (rc) return rc; }
        return 0;
    }
    // Scratch of the batch: per frame what lanes[0].keys / weights, d_wsorted and d_hist are to one build -- sized by the builds of THIS call
    // (n frames x the largest item bound among them: a host-known count, a gathered import's bound, or the set capacity for a pass
    // whose count only the device knows), not by the widest batch and the padded capacity the context could ever see: with an
    // uncalibrated cache (core_count x padding) 32 x capacity x 16 B would be gigabytes.  It only grows; spcbpt_lvc_set_capacity
    // and leaving light-ahead mode free it.  If the device cannot hold it the builds run one by one (build_sampler's own scratch).
    size_t stride = 1;
    for (int k = 0; k < n; k++) {
        const int b = pending[(size_t)k];
        const int count = sets[b].bound >= 0 ? sets[b].bound : sets[b].count_host;
        stride = std::max(stride, count < 0 ? lvc_capacity : std::min((size_t)count, lvc_capacity));
    }
    stride = (stride + 4095) / 4096 * 4096;
    if (!sbb_keys || sbb_frames < n || sbb_capacity < stride) {
        const int frames = std::max(n, sbb_frames);
        const size_t cap = std::max(stride, sbb_capacity);
        const size_t limit = sbb_debug_limit();   // tests: pretend the device refuses more than this many bytes of batch scratch
        const size_t bytes = (size_t)frames * cap * (sizeof(uint32_t) + sizeof(float) + sizeof(double));
        // (round 6, advisor) A size the device has refused is not asked for again until the capacity or the mode changes -- every call used
        // to repeat the device-wide wait, four hipMallocs and the failure path -- and the scratch that exists is kept while the larger one
        // is tried: a later, smaller batch still fits it.  The first refusal is reported once on stderr; spcbpt_get_pipeline_state's
        // callers see the count in spcbpt_debug_get("sbb_fallbacks").
        bool ok = bytes <= limit && (sbb_refused_bytes == 0 || bytes < sbb_refused_bytes);
        uint32_t* nk = nullptr; float* nw = nullptr; double* ns = nullptr; int* nh = nullptr;
        if (ok) {
            if (sync_all()) return SPCBPT_ERR_HIP;
            ok = dev_alloc(&nk, (size_t)frames * cap) == hipSuccess;
            ok = ok && dev_alloc(&nw, (size_t)frames * cap) == hipSuccess;
            ok = ok && dev_alloc(&ns, (size_t)frames * cap) == hipSuccess;
            ok = ok && dev_alloc(&nh, (size_t)frames * sampler_build_hist_ints()) == hipSuccess;
            if (!ok) { (void)hipGetLastError(); dev_free(nk); dev_free(nw); dev_free(ns); dev_free(nh); }   // (an allocation failure is sticky in hipGetLastError only)
        }
        if (!ok) {
            if (sbb_refused_bytes == 0 || bytes < sbb_refused_bytes) {
                if (sbb_refused_bytes == 0)
                    fprintf(stderr, "spcbpt: no room for %zu bytes of batched sampler-build scratch (%d frames x %zu vertices): building one by one\n", bytes, frames, cap);
                sbb_refused_bytes = bytes;
            }
            sbb_fallbacks++;
            for (int k = 0; k < n; k++) { const int rc = build_sampler(); if (rc) return rc; }
            return 0;
        }
        free_batch_build_scratch();
        sbb_keys.adopt(nk, (size_t)frames * cap); sbb_weights.adopt(nw, (size_t)frames * cap); sbb_wsorted.adopt(ns, (size_t)frames * cap);
        sbb_hist.adopt(nh, (size_t)frames * sampler_build_hist_ints());   // (the old scratch was kept while these were tried)
        sbb_frames = frames; sbb_capacity = cap;
    }
    SamplerBuildBatch B = {};
    B.keys = sbb_keys; B.weights = sbb_weights; B.wsorted = sbb_wsorted; B.hist = sbb_hist; B.item_stride = sbb_capacity;
    int built[kMaxBatchFrames];
    for (int k = 0; k < n; k++) {
        const int b = built[k] = pending[(size_t)k];
        CacheSet& S = sets[b];
        if (S.light_lane != 0 && S.light_counts_valid) HIP_TRY(this, S.light.wait_on(stream));   // traced on the second lane
        const bool dev_count = S.bound >= 0;   // gathered import: totals (and the path count) on the device, build over the upper bound
        if (dev_count) HIP_TRY(this, S.exch.wait_on(stream));
        int count = dev_count ? S.bound : S.count_host;
        const bool lazy = count < 0;   // a light pass's count: read on the device (no host wait for the pass)
        if (lazy) count = (int)std::min<size_t>(lvc_capacity, 0x7fffffff);
        // the path count: a light pass's compaction (and a gathered import) has left it in the set; only a cache that came some other way
        // (spcbpt_lvc_import) has it counted by the build, as build_sampler does
        const bool count_paths = !dev_count && !S.light_counts_valid;
        B.lvc[k] = S.lvc; B.n_host[k] = count; B.n_dev[k] = (dev_count || lazy) ? S.counts : nullptr; B.path_count[k] = count_paths ? S.counts + 1 : nullptr;
        B.sub[k] = S.subspace; B.jump[k] = S.jump; B.cmfs[k] = S.cmfs; B.lvc_sorted[k] = S.lvc_sorted; B.guide[k] = S.guide;
        if (count_paths) HIP_TRY(this, hipMemsetAsync(S.counts + 1, 0, sizeof(int), stream));
    }
    time_begin("sampler_build");
    launch_sampler_build_batch(B, n, stream);
    time_end();
    HIP_TRY(this, hipGetLastError());
    keys_ready = false;
    for (int k = 0; k < n; k++) { const int rc = sampler_built(built[k]); if (rc) return rc; }
    have_sampler = true;
    lvc_count = B.n_dev[n - 1] ? -1 : B.n_host[n - 1];   // the members describe the set built last, as after build_sampler (-1: only the device knows)
    return 0;
}

}  // namespace spc
