// The bucket film and its median-of-means resolve: k_film_buckets runs in front of a film merge and folds the frame's sample into
// bucket subframe % K of the pixels the merge is about to rewrite (buckets_pixel.h, the function spcbpt_film_buckets_update_host runs
// on the host); k_robust_resolve trims the pixel's bucket means by their Gini coefficient and tone-maps what is left.
// (kernel_config.h maps the other kernel files)
#include <hip/hip_runtime.h>

#include "eye_walk.h"
#include "kernel_config.h"
#include "kernels_buckets.h"

namespace spc {

// One lane per pixel, 8x8 tile per wave, four tiles per block: the launch shape of k_film_moments (lane_pixel), so that exactly the
// pixels of the launch's bands are touched.  Subframe 0 rewrites the pixel in all K planes, any other subframe in one.
__global__ __launch_bounds__(BLOCK) void k_film_buckets(const BucketParams p) {
    KParams q = {};
    q.width = p.width; q.height = p.height;
    q.row_begin = p.row_begin; q.row_end = p.row_end; q.row_step = p.row_step;
    uint32_t x, y;
    if (!lane_pixel(q, x, y)) return;
    const size_t px = (size_t)p.width * p.height, idx = (size_t)y * p.width + x;
    const float4 r = ldq(p.result, idx);
    const float s3[3] = {r.x, r.y, r.z};
    float4* planes = reinterpret_cast<float4*>(p.planes);
    const uint32_t b = p.subframe % (uint32_t)p.buckets;
    float m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (p.subframe == 0) {
        for (int k = 1; k < p.buckets; k++) planes[(size_t)k * px + idx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    } else {
        const float4 o = planes[(size_t)b * px + idx];
        m[0] = o.x; m[1] = o.y; m[2] = o.z; m[3] = o.w;
    }
    film_bucket_update(s3, m);
    planes[(size_t)b * px + idx] = make_float4(m[0], m[1], m[2], m[3]);
}

static int bucket_blocks(const BucketParams& p) {
    // one wave per 8x8 tile of the selected bands, four tiles per block (render_blocks of kernels.hip)
    const int tiles_x = ((int)p.width + 7) / 8;
    const int band_begin = p.row_begin / 8;
    const int band_end = (std::min(p.row_end, (int)p.height) + 7) / 8;
    const int step = p.row_step < 1 ? 1 : p.row_step;
    const int nb = band_end > band_begin ? (band_end - band_begin + step - 1) / step : 0;
    return (tiles_x * nb + (BLOCK / 64) - 1) / (BLOCK / 64);
}
void launch_film_buckets(const BucketParams& p, hipStream_t s) {
    const int blocks = bucket_blocks(p);
    if (blocks <= 0 || !p.result || !p.planes || !film_buckets_valid(p.buckets)) return;
    hipLaunchKernelGGL(k_film_buckets, dim3((unsigned)blocks), dim3(BLOCK), 0, s, p);
}

// One lane per pixel in index order: consecutive lanes read consecutive float4s of each plane (bucket-major), K loads per lane, all
// issued before the first use.  The buckets stay in registers for both passes (the rank counting and the kept sum), every index a
// compile-time constant of the loops unrolled over KP: no scratch, no LDS.
template <int KP>
__global__ __launch_bounds__(BLOCK) void k_robust_resolve(const RobustParams p) {
    const size_t px = (size_t)p.width * p.height;
    const size_t idx = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= px) return;
    float bk[KP][4];
#pragma unroll
    for (int i = 0; i < KP; i++) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i < p.buckets) v = ldq(p.planes, (size_t)i * px + idx);
        bk[i][0] = v.x; bk[i][1] = v.y; bk[i][2] = v.z; bk[i][3] = v.w;
    }
    float out[4];
    robust_resolve_pixel<KP>(bk, p.buckets, p.strength, out);
    reinterpret_cast<float4*>(p.out)[idx] = make_float4(out[0], out[1], out[2], out[3]);
    p.frame[idx] = film_tone_map(mk3(out[0], out[1], out[2]));   // film_write's tone map (device_lib.h)
}

void launch_robust_resolve(const RobustParams& p, hipStream_t s) {
    const size_t px = (size_t)p.width * p.height;
    if (px == 0 || !p.planes || !p.out || !p.frame || !film_buckets_valid(p.buckets)) return;
    const dim3 grid((unsigned)((px + BLOCK - 1) / BLOCK)), block(BLOCK);
    if (p.buckets <= 4) hipLaunchKernelGGL(k_robust_resolve<4>, grid, block, 0, s, p);
    else if (p.buckets <= 8) hipLaunchKernelGGL(k_robust_resolve<8>, grid, block, 0, s, p);
    else if (p.buckets <= 16) hipLaunchKernelGGL(k_robust_resolve<16>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(k_robust_resolve<32>, grid, block, 0, s, p);
}

}  // namespace spc
