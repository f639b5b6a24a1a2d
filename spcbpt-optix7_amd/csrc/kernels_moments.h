// Launchers of the film's second moment and of the error estimate (kernels_moments.hip).  Declared here and not in kernels.h, which
// is part of the eye megakernel's source hash (source_hash.py: KERNEL_SOURCES).
#pragma once
#include <hip/hip_runtime.h>

#include "moments_pixel.h"

namespace spc {

struct MomentsParams {  // passed by value as the kernel argument block of k_film_moments: the film-merge launch it runs in front of
    uint32_t width, height, subframe;
    int row_begin, row_end, row_step;   // the launch's 8-row bands (lane_pixel)
    const float* accum;                 // the film before the merge (read only)
    const float* result;                // the frame's samples (read only)
    float* m2n;                         // float4 per pixel: (M2_r, M2_g, M2_b, n)
};
void launch_film_moments(const MomentsParams& p, hipStream_t s);

// Film error: k_film_error leaves one partial (sum, maximum, count) per block in `partials`, k_film_error_final adds them in index
// order into `out` (int64 pixels, double mean, double max: spcbpt_film_error_stats).  No atomics: the same film gives the same bits.
static constexpr int kFilmErrorMaxBlocks = 1024;
struct FilmErrorPartial { double sum; float max; uint32_t count; };
int film_error_blocks(size_t pixels);
void launch_film_error(const float* accum, const float* m2n, size_t pixels, FilmErrorPartial* partials, void* out, hipStream_t s);

}  // namespace spc
