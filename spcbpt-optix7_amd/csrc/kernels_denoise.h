// Launchers of the a-trous denoiser (kernels_denoise.hip).  Declared here and not in kernels.h, which is part of the eye
// megakernel's source hash (source_hash.py: KERNEL_SOURCES).
#pragma once
#include <hip/hip_runtime.h>

#include "denoise_pixel.h"

namespace spc {

struct DenoiseParams {  // passed by value as the kernel argument block of k_demodulate / k_atrous / k_remodulate
    float U[3], V[3], W[3];
    uint32_t width, height;
    const float* accum;          // the film (read only)
    const float* albedo;         // feature buffers (read only)
    const float* normal_depth;
    float* position;             // float4 per pixel: X = d_c depth (written by k_demodulate)
    float* ping;                 // float4 per pixel: c_i, the two sides of the iteration
    float* pong;
    float* denoised;             // float4 per pixel: c_last x albedo, w = 1
    uint32_t* frame;             // RGBA8 per pixel: film_write's tone map of `denoised`
};

void launch_demodulate(const DenoiseParams& p, hipStream_t s);                                        // accum, features -> ping, position
void launch_atrous(const DenoiseParams& p, const AtrousStep& a, bool ping_to_pong, hipStream_t s);    // one iteration
void launch_remodulate(const DenoiseParams& p, bool from_pong, hipStream_t s);                        // c_last -> denoised, frame
// the variance-guided form (spcbpt_denoise_variance): the variance rides in the .w of ping / pong; launch_remodulate ends it too
void launch_demodulate_var(const DenoiseParams& p, const float* m2n, hipStream_t s);                      // accum, features, moments -> ping, position
void launch_atrous_var(const DenoiseParams& p, const AtrousVarStep& a, bool ping_to_pong, hipStream_t s); // one iteration
// spcbpt_history_denoise: the same start planes from the resolved image (in p.accum's place) and its variance plane; launch_atrous_var / launch_remodulate go on
void launch_demodulate_resolved(const DenoiseParams& p, const float* resolved_var, hipStream_t s);

}  // namespace spc
