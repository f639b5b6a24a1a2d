// Launcher of the batched film merge that keeps the film's second moment and its buckets (kernels_merge_stats.hip).  Declared here and
// not in kernels.h, which is part of the eye megakernel's source hash (source_hash.py: KERNEL_SOURCES).
#pragma once
#include <hip/hip_runtime.h>

#include "merge_stats_pixel.h"

namespace spc {

struct MergeStatsParams {  // passed by value as the kernel argument block of k_film_merge_batch_stats
    uint32_t width, height;
    int row_begin, row_end, row_step;               // the launch's 8-row bands (lane_pixel)
    int frames;                                     // n <= kMergeStatsMaxFrames
    int buckets;                                    // K, 0 = no buckets
    float* accum;                                   // the film's running mean, float4 per pixel
    uint32_t* frame;                                // RGBA8: the film's tone map of the last mean (may be null)
    float* m2n;                                     // (M2_r, M2_g, M2_b, n) per pixel, null = no moments
    float* planes;                                  // [K][height][width] float4: (mean_r, mean_g, mean_b, n)
    const float* result[kMergeStatsMaxFrames];      // per frame: its samples (read only)
    uint32_t subframe[kMergeStatsMaxFrames];
};
// m2n != null selects the moments, buckets != 0 the buckets; with neither nothing is launched (that merge is k_film_merge_batch's)
void launch_film_merge_batch_stats(const MergeStatsParams& p, hipStream_t s);

}  // namespace spc
