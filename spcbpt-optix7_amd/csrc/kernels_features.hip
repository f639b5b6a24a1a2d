// The first-hit feature pass: k_features shoots k_pt's primary ray through every pixel of the launch's rows and keeps albedo,
// normal and depth of what it hits (dev_features.h), as running means over the subframes like the film's.
// (kernel_config.h maps the other kernel files)
#include <hip/hip_runtime.h>

#include "dev_features.h"
#include "eye_walk.h"
#include "kernel_config.h"
#include "kernels_features.h"

namespace spc {

// One lane per pixel, 8x8 tile per wave, four tiles per block: the launch shape of k_pt (lane_pixel), and its ray -- camera_ray
// with the film's seed, so subframe 0 goes through the pixel centre and subframe k > 0 takes the jitter the film's sample of that
// subframe took.
__global__ __launch_bounds__(BLOCK, SPC_WAVES) void k_features(const FeatureParams p) {
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
    const f3 dir = camera_ray(q, x, y, seed, p.subframe);
    HitRec h;
    const bool hit = traverse<false, false>(S, st, ld3(p.eye), dir, kEps, 1e16f, h, cn);
    FeatureSample s = feature_sample(S, hit, h, dir);
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

static int feature_blocks(const FeatureParams& p) {
    // one wave per 8x8 tile of the selected bands, four tiles per block (render_blocks of kernels.hip)
    const int tiles_x = ((int)p.width + 7) / 8;
    const int band_begin = p.row_begin / 8;
    const int band_end = (std::min(p.row_end, (int)p.height) + 7) / 8;
    const int step = p.row_step < 1 ? 1 : p.row_step;
    const int nb = band_end > band_begin ? (band_end - band_begin + step - 1) / step : 0;
    return (tiles_x * nb + (BLOCK / 64) - 1) / (BLOCK / 64);
}
int feature_thread_count(const FeatureParams& p) { return feature_blocks(p) * BLOCK; }
void launch_features(const FeatureParams& p, hipStream_t s) {
    const int blocks = feature_blocks(p);
    if (blocks <= 0) return;
    hipLaunchKernelGGL(k_features, dim3((unsigned)blocks), dim3(BLOCK), 0, s, p);
}

}  // namespace spc
