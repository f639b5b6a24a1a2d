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

// the variance-carrying forms (spcbpt_history_denoise): the same planes plus one float4 variance plane (V_r, V_g, V_b, 0) beside each
struct ReprojectVarParams {   // ... of k_reproject_var
    ReprojectParams base;
    const float* hist_var;            // HV: the variance of H.rgb, taken at capture (read only)
    float* prior_var;                 // PV
};
struct ResolveVarParams {     // ... of k_resolve_var
    ResolveParams base;
    const float* prior_var;           // PV, or null with base.prior
    const float* m2n;                 // the film's moments plane (read only)
    float* out_var;                   // RV (spcbpt_history_resolve) or HV (spcbpt_history_capture)
};

void launch_reproject(const ReprojectParams& p, hipStream_t s);   // features, history -> prior
void launch_resolve(const ResolveParams& p, hipStream_t s);       // prior, film -> out (and its tone map)
void launch_reproject_var(const ReprojectVarParams& p, hipStream_t s);   // features, history, HV -> prior, PV in one pass
void launch_resolve_var(const ResolveVarParams& p, hipStream_t s);       // prior, PV, film, moments -> out, its variance (and its tone map)

}  // namespace spc
