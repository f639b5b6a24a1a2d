// Launchers of the bucket film and of its median-of-means resolve (kernels_buckets.hip).  Declared here and not in kernels.h, which
// is part of the eye megakernel's source hash (source_hash.py: KERNEL_SOURCES).
#pragma once
#include <hip/hip_runtime.h>

#include "buckets_pixel.h"

namespace spc {

struct BucketParams {  // passed by value as the kernel argument block of k_film_buckets: the film-merge launch it runs in front of
    uint32_t width, height, subframe;
    int row_begin, row_end, row_step;   // the launch's 8-row bands (lane_pixel)
    int buckets;                        // K
    const float* result;                // the frame's samples (read only)
    float* planes;                      // [K][height][width] float4: (mean_r, mean_g, mean_b, n)
};
void launch_film_buckets(const BucketParams& p, hipStream_t s);

struct RobustParams {  // the kernel argument block of k_robust_resolve
    uint32_t width, height;
    int buckets;                        // K
    float strength;
    const float* planes;                // the bucket planes (read only)
    float* out;                         // float4 per pixel: (r, g, b, w)
    uint32_t* frame;                    // RGBA8: the film's tone map of out.rgb
};
void launch_robust_resolve(const RobustParams& p, hipStream_t s);

}  // namespace spc
