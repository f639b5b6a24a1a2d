// Launchers of the local tone stage (kernels_local_tone.hip): the gather into the bilateral grid (one workgroup per node column), the
// grid blur and the slice with the gain.  Declared here and not in kernels.h, which is part of the eye megakernel's source
// hash (source_hash.py: KERNEL_SOURCES).
#pragma once
#include <hip/hip_runtime.h>

#include "local_tone_pixel.h"

namespace spc {

struct LocalToneParams {  // passed by value as the kernel argument block of the three kernels
    const float* src;     // float4 per pixel, rows in the film's order (read only)
    float* out;           // the local tone plane, float4 per pixel, the source's size
    float* grid[2];       // the two grid buffers, (A, B) per node, node (gx, gy, gz) at (gy GX + gx) NZ + gz
    int width, height;
    int cell, gx, gy, nz;
    float range, compress, detail, la;
};

void launch_local_tone_build(const LocalToneParams& p, int dst, hipStream_t s);                // the gather, into grid[dst]
void launch_local_tone_blur(const LocalToneParams& p, int src, hipStream_t s);                 // one blur pass, x then y then z: grid[src] -> grid[1 - src]
void launch_local_tone_slice(const LocalToneParams& p, int src, hipStream_t s);                // out = src lt_exp2(g), the base from grid[src]

}  // namespace spc
