// The light-tracing estimator "lt": k_lt_splat connects every vertex of the light-vertex cache to the camera and adds it to the
// pixel it lands on (BDPT strategy t = 1, which upstream disables: readme.md:27), k_lt_resolve hands the sum to the film.
// (kernel_config.h maps the other kernel files)
#include <hip/hip_runtime.h>

#include "dev_splat.h"
#include "eye_walk.h"
#include "kernel_config.h"
#include "kernels_splat.h"

namespace spc {

// Persistent waves like k_light_trace.  The cache is the queue: thread t looks at vertices t, t + T, t + 2 T, ... of the T threads
// launched (the count is read from device memory).  Most vertices of a cache are culled without a ray (outside the image, facing
// away, a zero BSDF value towards the eye), so a lane keeps culling until it HOLDS a live shadow ray or its share of the queue is
// dry, and only then does the wave enter the any-hit loop: one vertex per lane per traversal would run that loop at the few lanes
// whose vertex happened to survive.  A clear ray adds its contribution with three float atomics (12 B; a frame adds a few hundred
// thousand of them -- far below the chip's float-atomic rate, so nothing is pre-reduced on chip).  The sums depend on the order of
// arrival in the last bits: the film of "lt" is not bit-reproducible from run to run.
__global__ __launch_bounds__(BLOCK, SPC_WAVES) void k_lt_splat(const SplatParams p) {
    __shared__ uint32_t s_stack[BLOCK * STACK_LDS];
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
            live = splat_cull(p, *reinterpret_cast<const LightVertex*>(q), path_count, job);
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

int splat_block_threads() { return BLOCK; }
int splat_blocks(int max_blocks) { return max_blocks < 1 ? 1 : max_blocks; }
void launch_lt_splat(const SplatParams& p, int blocks, hipStream_t s) {
    if (blocks <= 0 || p.capacity <= 0) return;
    hipLaunchKernelGGL(k_lt_splat, dim3((unsigned)blocks), dim3(BLOCK), 0, s, p);
}
void launch_lt_resolve(const SplatParams& p, hipStream_t s) {
    // one wave per 8x8 tile of the selected bands, four tiles per block (render_blocks of kernels.hip)
    const int tiles_x = ((int)p.width + 7) / 8;
    const int band_begin = p.row_begin / 8;
    const int band_end = (std::min(p.row_end, (int)p.height) + 7) / 8;
    const int step = p.row_step < 1 ? 1 : p.row_step;
    const int nb = band_end > band_begin ? (band_end - band_begin + step - 1) / step : 0;
    const int blocks = (tiles_x * nb + (BLOCK / 64) - 1) / (BLOCK / 64);
    if (blocks <= 0) return;
    hipLaunchKernelGGL(k_lt_resolve, dim3((unsigned)blocks), dim3(BLOCK), 0, s, p);
}

}  // namespace spc
