// The light-tracing estimator "lt": k_lt_splat connects every vertex of the light-vertex cache to the camera and adds it to the
// pixel it lands on (BDPT strategy t = 1, which upstream disables: readme.md:27), k_lt_resolve hands the sum to the film.
// The ordered mode (spcbpt_set_splat_order) replaces the pair: k_lt_records does the same walk but STORES every vertex's contribution
// in the vertex's own slot, a stable radix sort by pixel (ctx_splat.hip) indexes the slots, and k_lt_gather sums every pixel's records
// in ascending cache order (splat_pixel.h) and hands the sum to the film -- the same bits on every run.
// (kernel_config.h maps the other kernel files)
#include <hip/hip_runtime.h>

#include "dev_splat.h"
#include "eye_walk.h"
#include "kernel_config.h"
#include "kernels_splat.h"
#include "splat_pixel.h"

namespace spc {

// Persistent waves like k_light_trace.  The cache is the queue: thread t looks at vertices t, t + T, t + 2 T, ... of the T threads
// launched (the count is read from device memory).  Most vertices of a cache are culled without a ray (outside the image, facing
// away, a zero BSDF value towards the eye), so a lane keeps culling until it HOLDS a live shadow ray or its share of the queue is
// dry, and only then does the wave enter the any-hit loop: one vertex per lane per traversal would run that loop at the few lanes
// whose vertex happened to survive.  A clear ray adds its contribution with three float atomics (12 B; a frame adds a few hundred
// thousand of them -- far below the chip's float-atomic rate, so nothing is pre-reduced on chip).  The sums depend on the order of
// arrival in the last bits: in this, the atomic mode, the film of "lt" is not bit-reproducible from run to run.
// LENS (spcbpt_set_lens with a radius > 0): splat_cull<true> connects every vertex to a lens point of its own; a kernel of its own
// (k_lt_splat_lens below), so that the pinhole launch runs the pinhole code.
template <bool LENS>
SPC_DEV void lt_splat_walk(const SplatParams& p, uint32_t* s_stack) {
    const DeviceScene& S = p.scene;
    const size_t gtid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    TravStack<BLOCK, STACK_LDS> st;
    st.init(s_stack, p.spill, p.spill_entries, gtid, p.diag);
    Counts<false> cn;
    const int n = min(p.sampler_counts[0], p.capacity);
    const float path_count = (float)p.sampler_counts[1];
    const size_t stride = (size_t)gridDim.x * BLOCK;
    size_t i = gtid;
    while (true) {
        SplatJob job;
        bool live = false;
        while (!live && i < (size_t)n) {
            const float4* src = reinterpret_cast<const float4*>(p.lvc + i);
            float4 q[6];
#pragma unroll
            for (int k = 0; k < 6; k++) q[k] = src[k];
            live = splat_cull<LENS>(p, *reinterpret_cast<const LightVertex*>(q), (uint32_t)i, path_count, job);
            i += stride;
        }
        if (!__any(live)) break;   // every lane's share of the queue is dry and nobody holds a ray
        if (live) {
            HitRec h;
            if (!traverse<true, false>(S, st, job.origin, job.dir, kEps, job.tmax, h, cn)) {
                float* dst = p.splat + (size_t)job.pixel * 4;
                atomicAdd(dst + 0, job.contrib.x);
                atomicAdd(dst + 1, job.contrib.y);
                atomicAdd(dst + 2, job.contrib.z);
            }
        }
    }
}
__global__ __launch_bounds__(BLOCK, SPC_WAVES) void k_lt_splat(const SplatParams p) {
    __shared__ uint32_t s_stack[BLOCK * STACK_LDS];
    lt_splat_walk<false>(p, s_stack);
}
__global__ __launch_bounds__(BLOCK, SPC_WAVES) void k_lt_splat_lens(const SplatParams p) {
    __shared__ uint32_t s_stack[BLOCK * STACK_LDS];
    lt_splat_walk<true>(p, s_stack);
}

// The splat buffer as this subframe's radiance: film_write into `result`, from where the ordinary film merge (k_film_merge: running
// mean by subframe, tone map) takes it -- read-back and accumulation behave as for every other algorithm.
__global__ __launch_bounds__(BLOCK) void k_lt_resolve(const SplatParams p) {
    KParams q = {};
    q.width = p.width; q.height = p.height; q.subframe = p.subframe;
    q.row_begin = p.row_begin; q.row_end = p.row_end; q.row_step = p.row_step;
    q.result = p.result;
    uint32_t x, y;
    if (!lane_pixel(q, x, y)) return;
    const float4 s = reinterpret_cast<const float4*>(p.splat)[(size_t)y * p.width + x];
    film_write(q, x, y, mk3(s.x, s.y, s.z));
}

// The ordered mode's first pass: the walk of k_lt_splat over slots [0, bound) instead of [0, n), bound >= n known to the host (the
// pattern of k_fill_keys_devcount).  Every slot is written exactly once per launch -- one 16-byte record (rgb, pixel bits), its sort
// key and its own index as the sort's value: by the lane that culls the vertex (pad key), by the lane that holds its shadow ray once the
// ray has been traced (the record, or the pad key when occluded), and for the slots [n, bound) by the lane whose turn they are (pad key).
// A slot's writer is its only writer, so there is nothing to zero beforehand and no atomic.  pad key = width * height: it sorts last.
SPC_DEV void splat_record_store(const SplatParams& p, uint32_t slot, f3 rgb, uint32_t key) {
    p.records[slot] = make_float4(rgb.x, rgb.y, rgb.z, __uint_as_float(key));
    p.keys[slot] = key;
    p.vals[slot] = slot;
}
// (LENS: a slot's lens point is a function of the slot and the subframe -- splat_cull -- so the records stay a function of the cache)
template <bool LENS>
SPC_DEV void lt_records_walk(const SplatParams& p, uint32_t* s_stack) {
    const DeviceScene& S = p.scene;
    const size_t gtid = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    TravStack<BLOCK, STACK_LDS> st;
    st.init(s_stack, p.spill, p.spill_entries, gtid, p.diag);
    Counts<false> cn;
    const size_t bound = (size_t)max(p.bound, 0);
    const size_t n = (size_t)max(min(min(p.sampler_counts[0], p.capacity), p.bound), 0);
    const float path_count = (float)p.sampler_counts[1];
    const uint32_t pad = p.width * p.height;
    const size_t stride = (size_t)gridDim.x * BLOCK;
    size_t i = gtid;
    while (true) {
        SplatJob job;
        bool live = false;
        while (!live && i < bound) {
            if (i < n) {
                const float4* src = reinterpret_cast<const float4*>(p.lvc + i);
                float4 q[6];
#pragma unroll
                for (int k = 0; k < 6; k++) q[k] = src[k];
                live = splat_cull<LENS>(p, *reinterpret_cast<const LightVertex*>(q), (uint32_t)i, path_count, job);
            }
            if (live) job.index = (uint32_t)i;
            else splat_record_store(p, (uint32_t)i, mk3(0.0f), pad);
            i += stride;
        }
        if (!__any(live)) break;   // every lane's share of the slots is written and nobody holds a ray
        if (live) {
            HitRec h;
            const bool clear = !traverse<true, false>(S, st, job.origin, job.dir, kEps, job.tmax, h, cn);
            splat_record_store(p, job.index, clear ? job.contrib : mk3(0.0f), clear ? job.pixel : pad);
        }
    }
}
__global__ __launch_bounds__(BLOCK, SPC_WAVES) void k_lt_records(const SplatParams p) {
    __shared__ uint32_t s_stack[BLOCK * STACK_LDS];
    lt_records_walk<false>(p, s_stack);
}
__global__ __launch_bounds__(BLOCK, SPC_WAVES) void k_lt_records_lens(const SplatParams p) {
    __shared__ uint32_t s_stack[BLOCK * STACK_LDS];
    lt_records_walk<true>(p, s_stack);
}

// The ordered mode's last pass, in place of k_lt_resolve: one lane per pixel of the launch's rows finds its segment in the sorted
// keys (one lower-bound search, then it runs while the key is its own), sums the segment's records in the order the stable sort left
// -- ascending cache index -- and hands the sum to the film.  A pixel without a record is +0.0f.
__global__ __launch_bounds__(BLOCK) void k_lt_gather(const SplatParams p) {
    KParams q = {};
    q.width = p.width; q.height = p.height; q.subframe = p.subframe;
    q.row_begin = p.row_begin; q.row_end = p.row_end; q.row_step = p.row_step;
    q.result = p.result;
    uint32_t x, y;
    if (!lane_pixel(q, x, y)) return;
    float acc[3];
    splat_segment_sum(p.keys_sorted, p.vals_sorted, (uint32_t)max(p.bound, 0), y * p.width + x, reinterpret_cast<const float*>(p.records), 4, acc);
    film_write(q, x, y, mk3(acc[0], acc[1], acc[2]));
}

int splat_block_threads() { return BLOCK; }
int splat_blocks(int max_blocks) { return max_blocks < 1 ? 1 : max_blocks; }
void launch_lt_splat(const SplatParams& p, int blocks, hipStream_t s) {
    if (blocks <= 0 || p.capacity <= 0) return;
    if (p.lens_radius > 0.0f) hipLaunchKernelGGL(k_lt_splat_lens, dim3((unsigned)blocks), dim3(BLOCK), 0, s, p);
    else hipLaunchKernelGGL(k_lt_splat, dim3((unsigned)blocks), dim3(BLOCK), 0, s, p);
}
void launch_lt_records(const SplatParams& p, int blocks, hipStream_t s) {
    if (blocks <= 0 || p.bound <= 0) return;
    if (p.lens_radius > 0.0f) hipLaunchKernelGGL(k_lt_records_lens, dim3((unsigned)blocks), dim3(BLOCK), 0, s, p);
    else hipLaunchKernelGGL(k_lt_records, dim3((unsigned)blocks), dim3(BLOCK), 0, s, p);
}
// one wave per 8x8 tile of the selected bands, four tiles per block (render_blocks of kernels.hip)
static int resolve_blocks(const SplatParams& p) {
    const int tiles_x = ((int)p.width + 7) / 8;
    const int band_begin = p.row_begin / 8;
    const int band_end = (std::min(p.row_end, (int)p.height) + 7) / 8;
    const int step = p.row_step < 1 ? 1 : p.row_step;
    const int nb = band_end > band_begin ? (band_end - band_begin + step - 1) / step : 0;
    return (tiles_x * nb + (BLOCK / 64) - 1) / (BLOCK / 64);
}
void launch_lt_resolve(const SplatParams& p, hipStream_t s) {
    const int blocks = resolve_blocks(p);
    if (blocks <= 0) return;
    hipLaunchKernelGGL(k_lt_resolve, dim3((unsigned)blocks), dim3(BLOCK), 0, s, p);
}
void launch_lt_gather(const SplatParams& p, hipStream_t s) {
    const int blocks = resolve_blocks(p);
    if (blocks <= 0) return;
    hipLaunchKernelGGL(k_lt_gather, dim3((unsigned)blocks), dim3(BLOCK), 0, s, p);
}

}  // namespace spc
