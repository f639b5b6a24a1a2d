// Launchers of the history reprojection (kernels_reproject.hip).  Declared here and not in kernels.h, which is part of the eye
// megakernel's source hash (source_hash.py: KERNEL_SOURCES).
#pragma once
#include <hip/hip_runtime.h>

#include "reproject_pixel.h"

namespace spc {

struct ReprojectParams {  // passed by value as the kernel argument block of k_reproject
    ReprojectCamera cur, hist;
    ReprojectStep step;
    uint32_t width, height;
    const float* normal_depth;        // the current view's feature plane (read only)
    const float* hist_normal_depth;   // G: the feature plane as it stood at capture (read only)
    const float* hist_rgbn;           // H: (rgb, n) at capture (read only)
    float* prior;                     // R: float4 per pixel, (rgb, m)
};

struct ResolveParams {    // ... of k_resolve
    uint32_t width, height;
    float frames;                     // Nf
    const float* prior;               // R, or null: no prior is live
    const float* accum;               // the film (read only)
    float* out;                       // float4 per pixel: the resolved image (spcbpt_history_resolve) or H (spcbpt_history_capture)
    uint32_t* frame;                  // RGBA8: the film's tone map of `out`, or null (capture)
};

void launch_reproject(const ReprojectParams& p, hipStream_t s);   // features, history -> prior
void launch_resolve(const ResolveParams& p, hipStream_t s);       // prior, film -> out (and its tone map)

}  // namespace spc
