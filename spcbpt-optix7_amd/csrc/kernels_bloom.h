// Launchers of the bloom stage (kernels_bloom.hip): the tiled down pass (level 0 with the threshold step fused in), the up-and-mix
// pass, the fused coarse tail (one workgroup runs the small end of the pyramid down and back up in LDS) and the composite.  Declared
// here and not in kernels.h, which is part of the eye megakernel's source hash (source_hash.py: KERNEL_SOURCES).
#pragma once
#include <hip/hip_runtime.h>

#include "bloom_pixel.h"

namespace spc {

// The fused tail keeps its levels in LDS as float4: 4 096 texels are the 64 KB a workgroup may declare.
static constexpr int kBloomTailTexels = 4096;
static constexpr int kBloomTailThreads = 1024;

struct BloomParams {  // passed by value as the kernel argument block of the four kernels
    const float* src;   // level 0: float4 per pixel, rows in the film's order (read only)
    float* out;         // the bloom plane, float4 per pixel, the source's size
    float* pyr;         // the pyramid scratch: float4 per texel, level k at texel offset off[k]
    int levels;
    float strength, threshold, clamp;
    int w[kBloomMaxLevels + 1], h[kBloomMaxLevels + 1];
    unsigned long long off[kBloomMaxLevels + 1];
    float g[kBloomMaxLevels + 1];
};

// The level the fused tail starts from: the smallest j in 1 .. levels - 1 whose coarser levels j + 1 .. levels fit the tail's LDS
// together and that itself holds at most `max_input` texels (one workgroup reads and rewrites it), 0 when there is none (levels == 1,
// or the coarsest level alone is too large).  The tail reads D_j from the scratch, builds D_{j+1} .. D_L and U_L .. U_{j+1} in LDS and
// leaves U_j in the scratch.  4 096: at 1920 x 1080, L = 6 the tail from level 5 (2 040 texels) measured 2 % under the per-level
// kernels, the tail from level 4 (8 160 texels, read and rewritten by one workgroup) level with them.
static constexpr size_t kBloomTailInputTexels = 4096;
int bloom_tail_from(const BloomParams& p, size_t max_input = kBloomTailInputTexels);

void launch_bloom_down(const BloomParams& p, int k, hipStream_t s);   // level k - 1 -> D_k (k = 1 reads src through the threshold step; k = levels stores g_L D_L)
void launch_bloom_up(const BloomParams& p, int k, hipStream_t s);     // U_k = g_k D_k + up(U_{k+1}), in place (k = 1 .. levels - 1)
void launch_bloom_tail(const BloomParams& p, int j, hipStream_t s);   // see bloom_tail_from
void launch_bloom_composite(const BloomParams& p, hipStream_t s);     // out = src + s (up(U_1) - P), alpha copied

}  // namespace spc
