// The per-pixel work of the film's second moment and of the error estimate built on it: one set of __host__ __device__ functions
// shared by k_film_moments / k_film_error (kernels_moments.hip) and the exported spcbpt_film_moments_update_host /
// spcbpt_film_error_host (moments_host.cpp, plain g++), so that both are testable without a GPU.  Float32 throughout, no
// contraction (the library's flags), the same operations on both sides.  Includes no device header (the denoise_pixel.h pattern).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SPC_MO_HD __host__ __device__ inline
#else
#define SPC_MO_HD inline
#endif

#include <math.h>
#include <stdint.h>

namespace spc {

// One merge of one pixel: `mean` is accum.rgb BEFORE the merge, `x` the frame's sample, m2n = (M2_r, M2_g, M2_b, n).
//   subframe == 0:  M2 = 0, n = 1                                (the film overwrites on subframe 0, so the moments restart)
//   subframe  > 0:  a = 1 / (float)(subframe + 1),  mean' = mean + a (x - mean)      (film_write's lerp3: the bits the merge stores)
//                   M2 += (x - mean) (x - mean'),  n += 1
// With subframes 0, 1, 2, ... in order this is Welford's update; like the film's own running mean it assumes that order.
SPC_MO_HD void film_moments_update(const float* mean, const float* x, uint32_t subframe, float* m2n) {
    if (subframe == 0) {
        m2n[0] = m2n[1] = m2n[2] = 0.0f;
        m2n[3] = 1.0f;
        return;
    }
    const float a = 1.0f / (float)(subframe + 1);
    for (int k = 0; k < 3; k++) {
        const float d = x[k] - mean[k];
        const float mean2 = mean[k] + a * d;
        m2n[k] += d * (x[k] - mean2);
    }
    m2n[3] += 1.0f;
}

// sd_k = sqrt(M2_k / (n (n - 1))): the standard error of the mean of channel k, n >= 2.  (x - mean) and (x - mean') have one sign
// up to the rounding of mean', so a sum of their products may sit a few ulp below zero where the samples are all but equal: max(., 0).
SPC_MO_HD void film_moments_sd(const float* m2n, float* sd) {
    const float nn = m2n[3] * (m2n[3] - 1.0f);
    for (int k = 0; k < 3; k++) sd[k] = sqrtf(fmaxf(m2n[k], 0.0f) / nn);
}

// e(p) = (0.3 sd_r + 0.6 sd_g + 0.1 sd_b) / (1e-2 + L(accum(p))) for n >= 2 (returns false, e untouched, otherwise): the relative
// standard error of the pixel's luminance with the channels taken as fully correlated (an upper bound); the film's luminance
// weights, the denoiser's floor.
SPC_MO_HD bool film_error_pixel(const float* accum, const float* m2n, float* e) {
    if (!(m2n[3] >= 2.0f)) return false;
    float sd[3];
    film_moments_sd(m2n, sd);
    const float lum = 0.3f * accum[0] + 0.6f * accum[1] + 0.1f * accum[2];
    *e = (0.3f * sd[0] + 0.6f * sd[1] + 0.1f * sd[2]) / (1e-2f + lum);
    return true;
}

}  // namespace spc
