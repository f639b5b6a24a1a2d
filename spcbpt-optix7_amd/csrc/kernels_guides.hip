// The reflected-guide pass: k_guides shoots k_features' primary ray through every pixel of the launch's rows, follows it through
// mirror-like surfaces (dev_guides.h, guide_step.h) and keeps albedo, normal and depth of the first surface that is not one, unfolded
// through the mirrors, as running means over the subframes like the first-hit planes'.
// (kernel_config.h maps the other kernel files)
#include <hip/hip_runtime.h>

#include "dev_guides.h"
#include "eye_walk.h"
#include "kernel_config.h"
#include "kernels_guides.h"

namespace spc {

// k_features' launch shape, ray and LDS traversal stack: one lane per pixel, 8x8 tile per wave, four tiles per block; camera_ray with
// the film's seed (with a lens set: the centre-of-lens ray, as the feature pass takes it).  A lane whose chain has ended sits out the
// remaining rounds; the loop is over when no lane of the wave is live (at most max_bounces + 1 segments).
__global__ __launch_bounds__(BLOCK, SPC_WAVES) void k_guides(const GuideParams p) {
    __shared__ uint32_t s_stack[BLOCK * STACK_LDS];
    KParams q = {};
    q.width = p.width; q.height = p.height; q.subframe = p.subframe;
    q.row_begin = p.row_begin; q.row_end = p.row_end; q.row_step = p.row_step;
#pragma unroll
    for (int k = 0; k < 3; k++) { q.U[k] = p.U[k]; q.V[k] = p.V[k]; q.W[k] = p.W[k]; }
    uint32_t x, y;
    if (!lane_pixel(q, x, y)) return;
    const DeviceScene& S = p.scene;
    TravStack<BLOCK, STACK_LDS> st;
    st.init(s_stack, p.spill, p.spill_entries, (size_t)blockIdx.x * BLOCK + threadIdx.x, p.diag);
    Counts<false> cn;
    uint32_t seed;
    f3 dir = camera_ray(q, x, y, seed, p.subframe);
    f3 origin = ld3(p.eye);
    GuideChain c;
    c.throughput = mk3(1.0f);
    c.length = 0.0f;
    c.M[0] = 1.0f; c.M[1] = 0.0f; c.M[2] = 0.0f;
    c.M[3] = 0.0f; c.M[4] = 1.0f; c.M[5] = 0.0f;
    c.M[6] = 0.0f; c.M[7] = 0.0f; c.M[8] = 1.0f;
    c.mirror_n = mk3(0.0f);
    c.bounces = 0;
    FeatureSample s;
    bool live = true;
    while (live) {
        HitRec h;
        const bool hit = traverse<false, false>(S, st, origin, dir, kEps, 1e16f, h, cn);
        live = guide_segment(S, p, hit, h, origin, dir, c, s);
    }
    const size_t idx = (size_t)y * p.width + x;
    float4* albedo = reinterpret_cast<float4*>(p.albedo);
    float4* normal_depth = reinterpret_cast<float4*>(p.normal_depth);
    if (p.subframe > 0) {
        const float a = 1.0f / (float)(p.subframe + 1);
        s.albedo = feature_mean(albedo[idx], s.albedo, a);
        s.normal_depth = feature_mean(normal_depth[idx], s.normal_depth, a);
    }
    albedo[idx] = s.albedo;
    normal_depth[idx] = s.normal_depth;
}

static int guide_blocks(const GuideParams& p) {
    // one wave per 8x8 tile of the selected bands, four tiles per block (feature_blocks of kernels_features.hip)
    const int tiles_x = ((int)p.width + 7) / 8;
    const int band_begin = p.row_begin / 8;
    const int band_end = (std::min(p.row_end, (int)p.height) + 7) / 8;
    const int step = p.row_step < 1 ? 1 : p.row_step;
    const int nb = band_end > band_begin ? (band_end - band_begin + step - 1) / step : 0;
    return (tiles_x * nb + (BLOCK / 64) - 1) / (BLOCK / 64);
}
int guide_thread_count(const GuideParams& p) { return guide_blocks(p) * BLOCK; }
void launch_guides(const GuideParams& p, hipStream_t s) {
    const int blocks = guide_blocks(p);
    if (blocks <= 0) return;
    hipLaunchKernelGGL(k_guides, dim3((unsigned)blocks), dim3(BLOCK), 0, s, p);
}

}  // namespace spc
