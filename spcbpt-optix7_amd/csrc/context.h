// Per-GPU context: owns every HBM buffer of the path (the reference leaves ownership to function-static
// thrust vectors and never frees, device_thrust.cu:287-293).
#pragma once
#include <hip/hip_runtime.h>

#include <deque>
#include <functional>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "layout.h"
#include "reproject_pixel.h"   // ReprojectCamera: the history keeps the camera it was captured under

namespace spc {

struct Preprocessor;
struct DenoiseParams;   // kernels_denoise.h

struct TimedSpan {
    std::string name;
    hipEvent_t a, b;
    hipStream_t s;
};

template <class T>
static hipError_t dev_alloc(T** p, size_t n) {
    *p = nullptr;
    if (n == 0) n = 1;
    return hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T));
}
template <class T>
static void dev_free(T*& p) {
    if (p) (void)hipFree((void*)p);
    p = nullptr;
}

// A grow-only device buffer that frees itself.  reserve() reallocates (contents lost) only when asked for more elements than it
// holds; like dev_alloc it never allocates nothing (0 elements -> 1).  The hipFree inside waits for the device by itself; a site
// that wants that wait spelled out calls sync_all() first.
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;   // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    hipError_t reserve(size_t n) {
        if (n == 0) n = 1;
        if (n <= cap) return hipSuccess;
        release();
        const hipError_t e = dev_alloc(&p, n);
        if (e == hipSuccess) cap = n;
        return e;   // (dev_alloc leaves p null when it fails)
    }
    void release() { dev_free(p); cap = 0; }
    void adopt(T* q, size_t n) { release(); p = q; cap = n; }   // takes over an allocation of n elements made with dev_alloc
    operator T*() const { return p; }
};

// An event and whether it has been recorded: waiting for one that never was is a no-op.
struct Event {
    hipEvent_t ev = nullptr;
    bool set = false;
    hipError_t record(hipStream_t s) {
        const hipError_t e = hipEventRecord(ev, s);
        if (e == hipSuccess) set = true;
        return e;
    }
    hipError_t wait_on(hipStream_t s) const { return set ? hipStreamWaitEvent(s, ev, 0) : hipSuccess; }
};

// One buffer set of the light-vertex cache: the compact cache of one light pass (or import) and the sampler tables built from it.
// What the eye pass reads exists once per frame in flight: Context::sets is a ring of n_sets of these.
struct CacheSet {
    DevBuf<LightVertex> lvc;
    DevBuf<LightVertex> lvc_sorted;   // the set's cache in its sampler's order (written by the sampler build, read by the eye megakernel)
    DevBuf<uint32_t> jump;
    DevBuf<float> cmfs;
    DevBuf<uint32_t> guide;           // the set's second-stage guide table (layout.h KParams::guide)
    DevBuf<DSubspace> subspace;
    int* counts = nullptr;            // [0] vertex_count, [1] path_count: a pointer into Context::d_set_counts_all
    Event light;                      // light pass + compaction of the set done (recorded on the stream of the pass's lane)
    Event sampler, render;
    // the event that marks the end of the last eye kernel that read the set: its own, or -- after a batched eye launch -- the ONE event
    // recorded for the whole batch (that of the batch's last set).  32 event records between a batch's eye kernel and its film merge
    // were 0.16 ms of idle GPU per launch (kernel trace of a long run).  Waiting on an event that has meanwhile been recorded again
    // waits for a LATER eye kernel -- more than needed, never a cycle: everything that kernel depends on was queued before it.
    int render_event_of = 0;
    Event on_stream;                  // last work queued on `stream` that reads or writes the set (sampler build, import copy):
                                      // a light pass on the second lane waits for it before it rewrites the set
    // Sharded job without host round trips (spcbpt_lvc_export_on / spcbpt_lvc_import_gathered, libspcbpt_mgpu): the all-gathered
    // shards are compacted on the exchange stream with the totals left on the DEVICE; the sampler build then runs over a host-known
    // upper bound (`bound`, pad keys sort behind the real items) instead of reading the count back.
    int bound = -1;                   // >= 0: the set's vertex count lives on the device only, this is its upper bound
    Event exch;                       // gathered compaction of the set done (recorded on the caller's exchange stream)
    int count_host = -1;              // vertex count of the set when the host knows it (after an import), else -1
    bool light_counts_valid = false;  // h_light_counts of the set describe its current contents
    int light_lane = 0;               // which lane's stream last wrote the set (its `light` event orders it)
};

// Second light lane.  On one in-order stream light pass, compaction, import copy and sampler build of consecutive frames
// form a chain of ~1.3 ms per frame -- more than a rank's share of the eye pass costs when the frame is sharded eight ways.
// With light passes running ahead, every other pass (kernel + compaction) therefore goes to a second stream with its own
// scratch, counts, key and temp buffers; imports and sampler builds stay on `stream` and wait for the pass's event.
// Lane 0 is Context::stream; its keys / vals / weights / temp are also the sampler build's, its spill area ensure_spill(., false)'s.
// Lane 1 is created on first use (ensure_lane_b): highest priority, non-blocking.
struct LightLane {
    hipStream_t stream = nullptr;
    DevBuf<LightVertex> scratch;               // core_count * core_padding
    DevBuf<int> core_counts, core_offsets;     // core_count + 1
    DevBuf<uint32_t> keys, vals;               // what the lane's compaction leaves (lane 0: valid for `keys_set` if keys_ready)
    DevBuf<float> weights;
    DevBuf<unsigned char> temp;
    DevBuf<uint32_t> spill;
    uint32_t* work_counter = nullptr;          // the lane's core queue: its word of d_work_counter
};

struct Context {
    int device = 0;
    hipStream_t stream = nullptr;    // light pass, sampler build, preprocessing, uploads
    // Render launches ("pt", "SPCBPT_eye") run on their own stream.  The eye megakernel ends with a drain phase (paths of up
    // to 50 bounces finishing with ever fewer live lanes: the average wave has left after 83 % of the kernel span), and the
    // light pass + sampler build of the NEXT frame do not depend on it.  With the sampler tables double-buffered, the host
    // loop launch("light trace") -> build_sampler -> launch("SPCBPT_eye") keeps its meaning while frame f+1's light pass
    // fills the idle machine under frame f's drain.  SPCBPT_OVERLAP=0 puts everything back on one stream.
    hipStream_t rstream = nullptr;              // = rstreams[rk], the stream of the render launch being issued
    hipStream_t cstream = nullptr;              // spcbpt_read_film's copies (created on first use)
    // Consecutive render launches alternate between two streams, each with its own work counter, spill area and `result`
    // buffer: frame f+1's eye kernel starts filling the machine while frame f's drains.  Only the film merges (running mean +
    // tone map from `result` into accum/frame) are chained, by ev_merge, so the image is the same as with one stream.
    // n_render streams are in use (default 2; SPCBPT_RENDER_STREAMS=1..8).  More frames in flight pay when one frame does not
    // fill the GPU -- a rank of an 8-GPU job renders 1/8 of the image but its frame still ends with the same 50-bounce chain.
    static const int kMaxRender = 8, kMaxSets = 128;
    int n_render = 2, n_sets = 6;   // n_sets = n_render + 4: one set per eye kernel in flight + the light passes ahead of them
    hipStream_t rstreams[kMaxRender] = {};
    int rk = 0, last_merge_k = -1;
    DevBuf<float> d_result[kMaxRender];
    Event ev_merge[kMaxRender];
    CacheSet sets[kMaxSets];
    int lset = 0, eset = 0;  // buffer set of the latest light pass, and of the sampler eye launches use
    // Light passes whose sampler has not been built yet, oldest first.  The host loop of a single GPU alternates
    // light pass -> sampler build, so the queue holds one set; a sharded job launches the NEXT frame's light pass before it
    // exchanges and builds the current one (the light pass is a 1 ms dependent chain however few paths it traces, and the
    // exchange makes the host wait for it), so export / import / build_sampler always address the OLDEST pending set.
    std::deque<int> pending;
    bool light_ahead = false;                // spcbpt_set_light_ahead: keep older unbuilt passes queued (default: only the latest)
    int keys_set = -1;                       // the set whose compaction left lanes[0].keys / vals / weights (valid if keys_ready)
    int export_on(hipStream_t xs, void** dv, void** dc, int* cap);
    int import_gathered(const void* shards, const int* counts_all, int world, int shard_cap, hipStream_t xs, int nf);
    int export_batch_on(hipStream_t xs, int nf, void* send, int* send_counts, int shard_cap);   // one exchange per light batch
    int wait_for_contents(hipStream_t xs, int s);
    hipEvent_t ev_import[2] = {};            // device-to-device import copies done (alternating: the caller alternates two staging buffers)
    long long import_gen = 0;
    int* h_import_counts = nullptr;          // pinned [kMaxSets][2]: source of the counts upload of an import (no host wait)
    int* h_light_counts = nullptr;           // pinned [kMaxSets][2]: (vertex_count, path_count) of a light pass, written on the lane's
                                             // stream before the set's `light` event -- the host reads them after waiting for that event only
    int build_set() const { return pending.empty() ? lset : pending.front(); }
    // The transitions of a buffer set, each written once (ctx_light.hip):
    int begin_rewrite(hipStream_t ls, int s, int& waited_for);   // `ls` waits for the set's readers before a light pass rewrites it
    void set_rewritten(int s);                                   // its sampler is gone, lane 0's keys no longer describe it
    int pass_traced(hipStream_t ls, int s, int lane);            // a light pass has been queued into it: unbuilt, at the back of `pending`
    int sampler_built(int s);                                    // its tables have been queued on `stream`: the set eye launches read
    void contents_imported(int s, int count_host, int bound);    // an import replaced its contents (ordered on `stream` / by `exch`)
    template <class P>
    void sampler_tables(P& d, int s) const {                     // the sampler-table pointers of a KParams / FrameDesc
        const CacheSet& S = sets[s];
        d.lvc = S.lvc; d.lvc_sorted = S.lvc_sorted; d.subspace = S.subspace; d.cmfs = S.cmfs; d.guide = S.guide; d.sampler_counts = S.counts;
        if constexpr (std::is_same<P, KParams>::value) d.jump = reinterpret_cast<const int32_t*>(S.jump.p);
    }
    LightLane lanes[2];
    int light_toggle = 0;
    int ensure_lane_b();   // lane 1 exists and matches the light-pass geometry and the set capacity
    // the light-pass fields of kp (geometry, frame, scratch, counts, counters) and the spill area of the grid that will run it:
    // n_frames == 0: one pass (or the probe), a thread per core; n_frames > 0: a batched pass of light_trace_blocks(kp, grid_cap) blocks
    int light_pass_params(uint32_t frame, int n_frames, LightVertex* scratch, int* core_counts, bool count_events, DevBuf<uint32_t>& spill, int grid_cap);
    // Batched light pass (spcbpt_launch_light_batch): the passes of n consecutive launch frames as ONE persistent launch on the
    // second lane, each into its own set.  A rank of an 8-GPU job traces 1/8 of the cores per frame; its pass is then a ~1.2 ms
    // chain of 50 dependent bounces that the few block slots beside the eye grid run one after the other -- eight of them per eye
    // batch cost more than the eye batch itself.  In one queue they regenerate like one pass of eight times the cores.
    // It has scratch, counts and spill of its own and uses lane 1's stream, temp and queue word.
    DevBuf<LightVertex> lb_scratch;                                   // n * core_count * core_padding
    DevBuf<int> lb_core_counts, lb_core_offsets, lb_path_counts;      // n * (core_count + 1); kMaxBatchFrames
    DevBuf<uint32_t> lb_spill;
    int launch_light_batch(uint32_t first_frame, int n);
    DevBuf<int> d_set_counts_all;            // one allocation behind the sets' `counts`: set s at + 2 s (a batch copies its sets' counts to the
                                             // host as ranges), and a spare pair behind them (probe_lvc_capacity)
    DevBuf<uint32_t> d_spill_rs[kMaxRender];   // traversal-stack spill areas of the render streams (lanes[0].spill serves `stream`)
    int sync_all();
    std::string error;
    KParams kp;
    // scene
    DevBuf<float> d_nodes;
    DevBuf<float> d_nodes_q;               // the same nodes in the quad-lane layout (quad_trace.hip), built on first use
    DevBuf<float> d_nodes_q2;              // ... with the scale exponents as signed bytes (the lean quad kernel)
    DevBuf<float> d_tris;
    int n_paired = 0;                      // triangles that are half of a fan pair (lbvh.h): what the pooled pass tests two at a time
    DevBuf<int32_t> d_tri_orig;
    DevBuf<DMaterial> d_mats;
    DLight* d_lights = nullptr;
    DevBuf<DTexture> d_tex;
    std::vector<uint32_t*> d_tex_data;
    int n_triangles = 0, n_nodes = 0, bvh_depth = 0, n_lights = 0, n_mats = 0;
    // environment map (params.sky; spcbpt_set_environment): device copies of the flipped texture and the sampling CMF
    float* d_env_tex = nullptr;
    float* d_env_cmf = nullptr;
    std::vector<DLight> h_lights;          // the light list as uploaded (the ENV light is appended to it)
    std::vector<float> h_etable;           // the emitter-triangle table of the mesh lights (layout.h), uploaded right behind the list
    std::vector<int> h_light_tris;         // per light: triangles that emit (2 for a quad)
    int upload_lights();                   // (re)allocates d_lights = h_lights + h_etable and points the kernels' scene at it
    float bbox_lo[3] = {0, 0, 0}, bbox_hi[3] = {0, 0, 0};   // of every vertex handed to spcbpt_create (+ the light quads)
    int set_environment(const float* rgba, int w, int h, const float* center, float radius);
    // film
    DevBuf<float> d_accum;
    DevBuf<uint32_t> d_frame;
    bool have_camera = false;
    // subspace tuple
    float* d_eye_tree = nullptr;
    float* d_light_tree = nullptr;
    DevBuf<float> d_Q;
    DevBuf<float> d_gamma;
    DevBuf<float> d_gamma2;      // three-level copy of d_gamma (layout.h: CMF2_ROW)
    DevBuf<float> d_gamma_q;     // Gamma / Q table (layout.h: KParams::gamma_q)
    DevBuf<uint16_t> d_guide1;   // first-stage guide table (layout.h: KParams::cmf_guide1)
    bool gamma_monotone = false; // every row of the installed matrix is a proper CMF: first-stage sampling may count instead of bisect
    std::vector<spcbpt_tree_node> h_eye_tree, h_light_tree;
    std::vector<float> h_Q, h_gamma;
    bool have_subspace = false;
    bool tree_has_direction = false;   // a caller-supplied classifier with direction nodes (type 2): labels depend on the viewing
                                       // direction, so the label-caching kernels do not apply (device_lib.h) and the generic
                                       // (counting) instantiations run instead
    // light pass + LVC + sampler
    spcbpt_light_trace_params lt = {100000, 52, 1, 0, 100000, 1};
    // Vertices every buffer set (compact LVC, jump buffer, CMFs) holds.  NOT the padded worst case num_core x core_padding (5.2 M
    // vertices = 541 MB per set at the bench geometry, 53 GB for the 99 sets of a 32-frame pipeline): a light pass fills ~5 % of
    // its padded slots, so the sets are sized from a PROBE pass -- the first light pass after spcbpt_set_light_trace is traced
    // once more into the padded scratch and counted on the host (start-up) -- as 2 x that count (scaled to the whole job's cores
    // for a rank of a sharded job), at most the worst case.  The compaction kernels cut a pass off at the capacity and raise
    // diag[2] (SPCBPT_ERR_CAPACITY at the next sync): the vertex count of 100 000 paths varies by a fraction of a per cent, so
    // the flag means a changed scene or tuple, and spcbpt_lvc_set_capacity fixes the size by hand.
    size_t lvc_capacity = 0;
    size_t lvc_fixed = 0;            // spcbpt_lvc_set_capacity / SPCBPT_LVC_CAPACITY: explicit capacity (0 = from the probe pass)
    bool lvc_probe_needed = false;   // set by set_light_trace, consumed by the next light pass
    int probe_lvc_capacity();
    DevBuf<uint32_t> d_keys2;        // the sampler build's own scratch (besides lanes[0].keys / vals / weights / temp), per vertex of a set
    DevBuf<double> d_wsorted, d_prefix;
    DevBuf<int> d_hist;               // per-block histograms / offsets of the four-launch sampler build (kernels.hip)
    bool counting_build = true;       // SPCBPT_SAMPLER_BUILD=hipcub selects the radix-sort form (same tables)
    int lvc_count = 0, path_count = 0;
    bool keys_ready = false, have_sampler = false;
    DevBuf<uint32_t> d_diag;           // KParams::diag: [0] dropped traversal-stack entries, [1] shard / gathered-cache overflow of exchange 1, [2] a light pass outgrew the set capacity
    int spill_entries_debug = -1;      // SPCBPT_DEBUG_SPILL_ENTRIES: caps the spill entries per thread (tests of the overflow report)
    int spill_entries_needed() const;  // 3 * bvh_depth - kStackLds (a 4-wide node pushes up to 3 children per level)
    int check_diag();                  // after a sync: SPCBPT_ERR_STATE if a kernel dropped stack entries since the last check
    // instrumentation
    DevBuf<uint32_t> d_work_counter;   // tile queues of the render streams, then the core queues of the two light lanes
    int num_cus = 0, blocks_per_cu[3] = {0, 0, 0};   // per kernel variant (single-frame launches), of the instantiation launched
    int blocks_per_cu_batch = 0;                       // the batched timed kernel's
    int blocks_per_cu_lens = 0;                        // the thin-lens form's (k_spcbpt_lens<ENV>, by scene.general as launched)
    int grid_percent = 0;              // persistent grid as a share of the resident block slots; 0 = 94 with several render streams, else 100 (launch_render)
    int light_blocks_wide = -1;        // ... of a pass that has the GPU to itself (no passes ahead): a lane per core, at most four blocks per CU (SPCBPT_LIGHT_BLOCKS_WIDE)
    int light_blocks = -1;             // persistent grid of the light pass (SPCBPT_LIGHT_BLOCKS; default: one block per CU)
    int light_batch_blocks = -1;       // ... of a batched light pass (SPCBPT_LIGHT_BATCH_BLOCKS; 0 = in proportion to the light paths per pixel, >= 16: launch_light_batch)
    int tiles_per_wave = 1;            // lower bound of 8x8 tiles per persistent wave (SPCBPT_TILES_PER_WAVE)
    DevBuf<unsigned long long> d_counters;
    bool counting = false, timing = false;
    bool count_executed = false;       // spcbpt_enable_counters(ctx, 2): count with the TIMED kernels' instantiations (label caching) instead of the reference's order
    int kernel_variant() const { return tree_has_direction ? 1 : (counting ? (count_executed ? 2 : 1) : 0); }   // kernels.h: launch_spcbpt
    std::vector<TimedSpan> spans;
    std::map<std::string, std::pair<double, int>> times;

    ~Context();
    void time_begin(const char* name, hipStream_t s = nullptr);
    void time_end();
    void resolve_spans();
    int ensure_spill(size_t threads, bool render = false);
    int ensure_temp(size_t bytes);
    int ensure_lvc_capacity(size_t n);
    int upload_tree(const spcbpt_tree_node* t, int n, float*& d_tree, std::vector<spcbpt_tree_node>& host_copy);
    int install_subspace(const spcbpt_tree_node* et, int ne, const spcbpt_tree_node* lt, int nl, const float* q, const float* g);
    int install_minimal_tuple();
    int set_light_trace(const spcbpt_light_trace_params& p);
    int launch_light(uint32_t frame);
    int fetch_counts();           // counts of the latest light pass's set (lset) -> lvc_count, path_count
    int fetch_counts_of(int set);
    int build_sampler();
    int build_sampler_batch(int n);   // the n oldest pending passes in one set of four launches (capi.hip)
    DevBuf<uint32_t> sbb_keys; DevBuf<float> sbb_weights; DevBuf<double> sbb_wsorted; DevBuf<int> sbb_hist;   // its scratch: per frame what lanes[0].keys .. d_hist are
    int sbb_frames = 0; size_t sbb_capacity = 0;   // frames x items per frame it holds
    int sbb_fallbacks = 0;                          // batches built one by one because the scratch could not be allocated
    size_t sbb_refused_bytes = 0;                   // the smallest scratch size the device has refused (0: none): not asked for again until the capacity or the mode changes
    void free_batch_build_scratch();
    size_t sbb_debug_limit() const;
    // the tables of the last sampler build are still what that build left (no later pass, import or re-allocation took the set)
    bool sampler_intact() const { return !built_sets.empty() && built_sets.back() == eset && sets[eset].sampler.set; }
    int launch_render(const char* name, bool spcbpt_alg, uint32_t frame, int r0, int r1, int rs, bool full_mis = false, bool defer_merge = false);
    // spcbpt_launch_deferred: a render launch whose film merge (running mean + tone map from its `result` buffer) has not been queued:
    // the frame is either merged later (merge_deferred(true)) or never (false) -- the interactive loop's speculative next frame
    struct Deferred { bool active = false; int rk = 0; uint32_t subframe = 0; int row_begin = 0, row_end = 0, row_step = 1; float* result = nullptr; } deferred;
    int merge_deferred(bool keep);
    int sync_film();
    // Batched eye launch (spcbpt_launch_eye_batch): the last n built samplers, one per frame, rendered by ONE persistent kernel
    // whose tile queue spans the frames (kernels.hip: BATCH).  A rank's share of a sharded frame is a few thousand tiles --
    // about one per resident wave, i.e. all drain phase; four frames in one queue regenerate like one frame four times the size.
    std::deque<int> built_sets;                                  // sets of the most recent sampler builds, oldest first
    int eye_batch = 1;                                           // frames per batched launch the context is sized for (SPCBPT_EYE_BATCH)
    DevBuf<float> d_result_b[kMaxRender][kMaxBatchFrames];       // per render stream and frame slot: radiance of that frame
    DevBuf<FrameDesc> d_frames[kMaxRender];                      // device copies of the batch descriptors
    static const int kDescRing = 4;
    FrameDesc* h_frames = nullptr;                               // pinned [kMaxRender][kDescRing][kMaxBatchFrames]: descriptor uploads in flight
    hipEvent_t ev_desc[kMaxRender][kDescRing] = {};              // upload out of that pinned slot done
    int desc_gen[kMaxRender] = {};
    int launch_eye_batch(int n, const uint32_t* subframes, int r0, int r1, int rs);
    // ... and the same launch whose merge keeps the film's second moment and fills its buckets (spcbpt_launch_eye_batch_film;
    // kernels_merge_stats.hip).  batch_render is the body the two share: everything up to the merge, which `film` selects.
    int launch_eye_batch_film(int n, const uint32_t* subframes, int r0, int r1, int rs);
    int batch_render(const char* name, bool film, int n, const uint32_t* subframes, int r0, int r1, int rs);
    // "lt" (ctx_splat.hip): the cache of set `eset` splatted onto the film.  One splat buffer (float4 per pixel, summed with float
    // atomics) per render stream, allocated at the first "lt" launch of that stream after a resize.
    DevBuf<float> d_splat[kMaxRender];
    int launch_splat(uint32_t frame, int r0, int r1, int rs);
    // Thin-lens camera (ctx_lens.hip; spcbpt_set_lens): the two numbers live in kp (lens_radius, lens_focus), which spcbpt_set_camera* and
    // spcbpt_resize leave alone.  radius 0, the default, is the pinhole: every launcher then picks the kernels it always picked.
    int set_lens(float radius, float focus);
    void update_lens_axes();
    int debug_lens_rays(uint32_t subframe, float* out8);
    // The ordered mode of "lt" (spcbpt_set_splat_order, off by default): every vertex's contribution stored in the vertex's own slot,
    // a stable radix sort of (pixel, slot) and a per-pixel sum in slot order -- no atomics, the same film bits on every run.  Per render
    // stream and cache slot 32 B (a float4 record, the sort's key and value double buffers) plus hipcub's temporary storage and 4 B for
    // the launch's vertex count; allocated at the first ordered launch of the stream, grow-only with the cache capacity, released when
    // the mode goes back to atomic and at destroy: a context that never asks keeps its footprint, its launches and its film bits.
    struct SplatOrdered {
        DevBuf<float> records;                        // float4 per slot: (rgb, bits of the pixel index or of the pad key)
        DevBuf<uint32_t> keys, vals, keys2, vals2;    // the sort's input (written by k_lt_records) and output
        DevBuf<unsigned char> temp;
        DevBuf<int> count;                            // sampler_counts[0] of the set the last launch read, copied behind that launch
        void release() { records.release(); keys.release(); vals.release(); keys2.release(); vals2.release(); temp.release(); count.release(); }
    } d_ordered[kMaxRender];
    int splat_order = 0;              // SPCBPT_SPLAT_ATOMIC / SPCBPT_SPLAT_ORDERED
    int splat_records_rk = -1;        // the render stream whose buffers hold the last ordered launch's records (-1: none since the last resize)
    int splat_records_capacity = 0, splat_records_pixels = 0;   // ... the cache capacity and the pad key of that launch
    int set_splat_order(int mode);
    int splat_bound(int capacity);    // a host-known upper bound of set eset's vertex count, found without a host wait
    int read_splat_records(float* rgb, int32_t* pixel, int capacity, int* count);
    // Prologue and epilogue of the launches that end in a film merge (ctx_render.hip)
    int film_ready();                          // no deferred frame outstanding, a film, a camera
    int begin_render(int r0, int r1, int rs);  // the band of rows into kp, then the next render stream
    void next_render_stream();                 // consecutive render launches rotate through the render streams
    int chain_wait();    // `rstream` behind the last link of the film-merge chain
    int chain_end();     // ... and this launch as the chain's last link
    template <class Run>
    int chain_link(Run run) {   // one whole link: `run` queues its launches on `rstream`; a refusal of its own ends the call, not the link
        next_render_stream();
        if (int rc = chain_wait()) return rc;
        if (int rc = run()) return rc;
        return chain_end();
    }
    int render_done(int s);   // the eye kernel just queued on `rstream` is the last reader of set s
    int finish_frame();
    // First-hit feature buffers and the denoiser's planes (ctx_features.hip): float4 per pixel each, allocated at the first feature
    // launch / the first denoise after a resize (spcbpt_resize frees them), so a context that asks for neither keeps its footprint.
    DevBuf<float> d_feat_albedo, d_feat_normal_depth;                 // running means of (base colour, coverage) / (normal, depth)
    DevBuf<float> d_dn_position, d_dn_ping, d_dn_pong, d_denoised;
    DevBuf<uint32_t> d_denoised_frame;                                // RGBA8: the film's tone map of d_denoised
    bool have_features = false, have_denoised = false;                // ... since the last resize
    int launch_features(uint32_t subframe, int r0, int r1, int rs);
    int denoise(const spcbpt_denoise_params& p);
    // The driver of the three denoisers (denoise, denoise_variance, history_denoise), after the preconditions of each.  denoise_begin: the
    // parameter refusals under the caller's name, then the link begins.  denoise_run: the five planes, the span `who` -- `demodulate`
    // (the caller's launch, from `input`), the a-trous passes of either form, k_remodulate --, have_denoised and the end of the link.
    int denoise_begin(const char* who, const spcbpt_denoise_params& p);
    int denoise_run(const char* who, const spcbpt_denoise_params& p, float sigma_c_default, const float* input, bool variance_guided,
                    const std::function<void(const DenoiseParams&)>& demodulate, const float* albedo = nullptr, const float* normal_depth = nullptr);
    void free_features();
    // Reflected guides (ctx_guides.hip; spcbpt_launch_guides): a second pair of float4 planes, the first-hit planes' layout, filled by
    // k_guides with what the first surface that is not mirror-like shows along the primary ray's chain of reflections.  Allocated (zeroed)
    // at the first guide launch after a resize, freed by spcbpt_resize.  denoise_guides (spcbpt_set_denoise_guides; it outlives a resize)
    // makes spcbpt_denoise and spcbpt_denoise_variance -- and nothing else -- read them in place of the first-hit planes.
    DevBuf<float> d_guide_albedo, d_guide_normal_depth;
    bool have_guides = false;                                         // ... since the last resize
    int denoise_guides = SPCBPT_GUIDES_FIRST_HIT;
    int launch_guides(uint32_t subframe, int r0, int r1, int rs, const spcbpt_guide_params& gp);
    int denoise_planes(const char* who, const float*& albedo, const float*& normal_depth);   // the pair the switch selects, or the refusal
    void free_guides();
    // Second moment of the film (ctx_moments.hip; spcbpt_set_film_moments, off by default): one float4 per pixel (M2_r, M2_g, M2_b, n),
    // updated by k_film_moments in front of every film merge of finish_frame.  Allocated (zeroed) at the first merge after a resize
    // while the switch is on, freed by spcbpt_resize and by turning the switch off: a context that does not ask keeps its footprint,
    // its launches and its film bits.
    bool film_moments = false;
    DevBuf<float> d_m2n;
    DevBuf<unsigned char> d_err_scratch;   // film_error's per-block partials, then its 24-byte result
    int set_film_moments(bool on);
    int moments_step();                    // finish_frame: the update of this launch's pixels, queued on `rstream` in front of the merge
    int film_error(spcbpt_film_error_stats* out);
    int denoise_variance(const spcbpt_denoise_params& p);
    void free_moments();
    // Bucket film (ctx_buckets.hip; spcbpt_set_film_buckets, off by default): K float4 planes [K][height][width] of (mean_r, mean_g,
    // mean_b, n), bucket subframe % K updated by k_film_buckets in front of every film merge of finish_frame, and the two planes of
    // spcbpt_robust_resolve (float4 + RGBA8).  Allocated (zeroed) at the first merge or resolve after a resize while the switch is on,
    // freed by spcbpt_resize, by switching off and by changing K: a context that does not ask keeps its footprint, its launches and
    // its film bits.
    int film_buckets = 0;                  // K: 0 (off) or 3 .. 32
    DevBuf<float> d_buckets, d_robust;
    DevBuf<uint32_t> d_robust_frame;
    bool have_robust = false;              // a resolve since the planes were last freed
    int set_film_buckets(int k);
    int ensure_buckets(hipStream_t s);
    int buckets_step();                    // finish_frame: the update of this launch's pixels, queued on `rstream` in front of the merge
    int robust_resolve(float strength);
    void free_buckets();
    // The image-space stages (display, bloom, local tone) take one of the context's linear float4 images -- SPCBPT_DISPLAY_FILM .. _LOCAL,
    // resolved by linear_image (ctx_display.hip), which words every refusal of a source under the stage's name `who` -- or an image of
    // the caller's (spcbpt_*_image): caller_image refuses a null or mis-sized one, image_link is the link over a scratch copy of it.
    // The ONE scratch copy serves the three stages: every use is a chain link, so its upload runs behind every kernel of the link
    // before it, the call returns only when the upload is done, and a reserve that has to grow goes through hipFree, which waits for
    // the device.  Grow-only (16 B per pixel of the largest image given), allocated at the first such call, freed by spcbpt_resize.
    struct LinearImage {
        const float* p = nullptr;
        int width = 0, height = 0;
    };
    struct Plane {   // a float4 plane at the size of the image it was made from
        bool have = false;           // ... since the last resize
        int width = 0, height = 0;
    };
    DevBuf<float> d_stage_src;
    int linear_image(const char* who, int source, int last_source, LinearImage* out);
    int caller_image(const char* who, const float* rgba, int width, int height);
    int stage_upload(const float* rgba, int width, int height);   // inside a link: into d_stage_src on `rstream`, and waited for
    int read_plane(const char* stage, const Plane& b, const float* plane, float* rgba, int* width, int* height);   // spcbpt_read_bloom / _local_tone
    template <class Run>
    int image_link(const float* rgba, int width, int height, Run run) {
        return chain_link([&]() -> int {
            if (int rc = stage_upload(rgba, width, height)) return rc;
            return run(d_stage_src.p);
        });
    }
    // Display transform (ctx_display.hip; spcbpt_display / spcbpt_display_image, opt-in): an RGBA8 plane of its own and the device record
    // of kernels_display.h (histogram counters + adaptation state, 1 040 B).  Allocated at the first call, the plane grow-only;
    // spcbpt_resize frees both (and with the record the previous EV).  A context that does not ask keeps its footprint, its launches and
    // every plane's bits.
    DevBuf<uint32_t> d_display_frame, d_display_state;
    struct Display {
        bool have = false, have_hist = false, auto_ev = false;   // of the last call
        int width = 0, height = 0;                               // ... the size of the image it showed
        float ev = 0.0f;                                         // ... its EV, when that was the caller's
    } display_last;
    int display(int source, const spcbpt_display_params& p);
    int display_image(const float* rgba, int width, int height, const spcbpt_display_params& p);
    int display_run(const float* src, int width, int height, const spcbpt_display_params& p);   // the launches, on `rstream` inside a chain link
    int display_reset();
    void free_display();   // ... and the stages' scratch copy
    // Bloom (ctx_bloom.hip; spcbpt_bloom / spcbpt_bloom_image, opt-in): a float4 plane of its own at the size of the image it was made
    // from and the pyramid scratch (float4 per texel of the levels 1 .. L: about a third of the image).  Allocated at the first call,
    // grow-only; spcbpt_resize frees both.  A context that does not ask keeps its footprint, its launches and every plane's bits.
    DevBuf<float> d_bloom, d_bloom_pyr;
    Plane bloom_last;
    int bloom(int source, const spcbpt_bloom_params& p);
    int bloom_image(const float* rgba, int width, int height, const spcbpt_bloom_params& p);
    int bloom_run(const float* src, int width, int height, const spcbpt_bloom_params& p);   // the launches, on `rstream` inside a chain link
    void free_bloom();
    // Local tone mapping (ctx_local_tone.hip; spcbpt_local_tone / spcbpt_local_tone_image, opt-in): a float4 plane of its own at the size
    // of the image it was made from and the two grid buffers the gather and the blur passes go back and forth between (two floats per
    // node, (W / cell + 2)(H / cell + 2)(32 / range + 2) nodes: 2.3 MB each at 1920 x 1080 with the defaults).  Allocated at the first
    // call, grow-only; spcbpt_resize frees all three.  A context that does not ask keeps its footprint, its launches and every plane's bits.
    DevBuf<float> d_local, d_local_grid[2];
    Plane local_last;
    int local_tone(int source, const spcbpt_local_tone_params& p);
    int local_tone_image(const float* rgba, int width, int height, const spcbpt_local_tone_params& p);
    int local_tone_run(const float* src, int width, int height, const spcbpt_local_tone_params& p);   // the launches, on `rstream` inside a chain link
    void free_local_tone();
    // Adaptive sampling (ctx_adaptive.hip; spcbpt_adaptive_*): between adaptive_begin and adaptive_end / resize / clear_accum the film is
    // merged tile by tile, every 8x8 tile at a sample index of its own.  Per tile of the film a count (uint32) and an error (float, with
    // the number of pixels it is the mean of), a tile list (uint32, strictly ascending) and its length: 16 B per tile and 4 B, allocated
    // by adaptive_begin, freed when the mode ends.  The counts live on the device only; the list's length is known to the host.
    struct Adaptive {
        bool active = false;
        int tiles_x = 0, tiles_y = 0, n_listed = 0;
        DevBuf<uint32_t> samples, known, list, n_dev;
        DevBuf<float> error;
        int blocks_per_cu[2] = {0, 0};   // of k_spcbpt_tiles<ENV>, by scene.general
    } adaptive;
    int uniform_merge_allowed(const char* what);   // SPCBPT_ERR_STATE while adaptive sampling is active: launches that merge with one weight for all pixels
    int adaptive_begin(uint32_t frames);
    void adaptive_drop();                          // the mode ends, the buffers go (the caller has synchronised)
    int adaptive_select(const spcbpt_adaptive_params& ap, int* n_selected);
    int adaptive_set_tiles(const uint32_t* tiles, int n);
    int launch_adaptive(const char* alg);
    int read_adaptive(uint32_t* tile_samples, float* tile_error, uint32_t* tiles, int capacity, int* n);
    // History reprojection (ctx_history.hip; spcbpt_history_*): H = (rgb, n) and G = (normal, depth) as captured, the prior R of the
    // current view, the resolved image and its RGBA8 frame -- 68 B per pixel, allocated at the first capture after a resize or a reset
    // (a resolve without a capture allocates the last two only), freed by spcbpt_resize and spcbpt_history_reset.
    DevBuf<float> d_hist_rgbn, d_hist_normal_depth, d_prior, d_resolved;
    DevBuf<uint32_t> d_resolved_frame;
    ReprojectCamera hist_camera = {};
    uint32_t hist_width = 0, hist_height = 0;
    bool have_history = false, prior_live = false, have_resolved = false;
    int history_ready(const char* what, bool need_features);
    int resolve_into(uint32_t frames, float* out, uint32_t* frame, float* out_var = nullptr);   // out_var: the variance-carrying kernel
    int history_capture(uint32_t frames);
    int history_reproject(const spcbpt_reproject_params& p);
    int history_resolve(uint32_t frames);
    void free_history();
    // The variance of what is shown (spcbpt_history_denoise): HV, PV and RV, one float4 plane (V_r, V_g, V_b, 0) beside H, the prior and
    // the resolved image -- 48 B per pixel more, each allocated at the first call that writes it.  The history carries variance exactly
    // while the moments switch is on: a capture then writes HV, a reproject of a history with HV writes PV, a resolve writes RV.
    // Freed with the history planes; the flags fall with have_history / prior_live / have_resolved and with the moments switch.
    DevBuf<float> d_hist_var, d_prior_var, d_resolved_var;
    bool have_hist_var = false, have_prior_var = false, have_resolved_var = false;
    bool history_variance_now() const;   // the call being made carries variance
    int history_denoise(const spcbpt_denoise_params& p);
    // preprocess.hip
    Preprocessor* pre = nullptr;
    spcbpt_pretrace_path* d_pre_paths = nullptr;
    spcbpt_pretrace_node* d_pre_nodes = nullptr;
    size_t pre_capacity = 0;
    int pre_num_core = 100000, pre_padding = 10, pre_last_added = 0;
    int set_pretrace(int num_core, int padding);
    int launch_pretrace(uint32_t iteration);
    int preprocess_stage(int stage, int arg);
    int preprocess(int target_paths, int target_q_paths, bool train);
    void free_preprocess();
};

}  // namespace spc
