// The per-pixel work of a batched film merge that keeps the film's second moment and its buckets: one __host__ __device__ function
// shared by k_film_merge_batch_stats (kernels_merge_stats.hip) and the exported spcbpt_film_merge_batch_host (merge_stats_host.cpp,
// plain g++), so that both are testable without a GPU.  Float32 throughout, no contraction (the library's flags), the same
// operations in the same order on both sides.  Includes no device header (the moments_pixel.h / buckets_pixel.h pattern); the two
// updates themselves are those headers' functions.
#pragma once
#include "buckets_pixel.h"
#include "moments_pixel.h"

#if defined(__HIPCC__)
#define SPC_MS_HD __host__ __device__ inline
#else
#define SPC_MS_HD inline
#endif

namespace spc {

static constexpr int kMergeStatsMaxFrames = 32;   // = kMaxBatchFrames (layout.h)

// One pixel, the frames k = 0 .. n - 1 of a batch in that order; per frame what k_film_moments, then k_film_buckets, then k_film_merge
// do to the pixel in a launch of that frame alone:
//   MOMENTS:  film_moments_update(c, x_k, subframe_k, m2n)            (c: the mean BEFORE this frame's merge; restarts at subframe 0)
//   BUCKETS:  subframe_k == 0: every bucket of the pixel to zero;   film_bucket_update(x_k, bucket subframe_k % K)
//   the mean: subframe_k == 0: c = x_k;   else a = 1 / (float)(subframe_k + 1),  c = c + a (x_k - c)      (film_write's lerp3)
// sample(k, x) fills x[3] with frame k's sample of the pixel; bucket.load(b, m) / bucket.store(b, m) move the pixel's entry
// (mean_r, mean_g, mean_b, n) of plane b between the caller's memory -- of which this call is the only writer -- and m[4].  c[3] and
// m2n[4] are the caller's copies (they need no defined value on entry if subframe_0 == 0: the frame overwrites them).
template <bool MOMENTS, bool BUCKETS, class Sample, class Bucket>
SPC_MS_HD void film_merge_stats_pixel(int n, const uint32_t* subframe, Sample sample, int K, Bucket bucket, float* c, float* m2n) {
    // (the reads run ahead of the arithmetic they feed -- frame k + 1's sample and frame k's bucket are on their way while frame k's
    // moments are updated: on the device two loads in flight per lane instead of two round trips per frame; the values and the order
    // of the operations on them are the ones above)
    float next[3];
    sample(0, next);
    for (int k = 0; k < n; k++) {
        const float x[3] = {next[0], next[1], next[2]};
        if (k + 1 < n) sample(k + 1, next);
        const uint32_t sf = subframe[k];
        const int b = BUCKETS ? (int)(sf % (uint32_t)K) : 0;
        float m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (BUCKETS && sf != 0) bucket.load(b, m);
        if (MOMENTS) film_moments_update(c, x, sf, m2n);
        if (BUCKETS) {
            if (sf == 0) {
                const float zero[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int z = 0; z < K; z++)
                    if (z != b) bucket.store(z, zero);
            }
            film_bucket_update(x, m);
            bucket.store(b, m);
        }
        if (sf == 0) {
            c[0] = x[0]; c[1] = x[1]; c[2] = x[2];
        } else {
            const float a = 1.0f / (float)(sf + 1);
            for (int j = 0; j < 3; j++) c[j] = c[j] + a * (x[j] - c[j]);
        }
    }
}

}  // namespace spc
