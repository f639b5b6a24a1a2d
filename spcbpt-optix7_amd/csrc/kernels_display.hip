// The display transform: k_display_histogram counts the image's luminances into the 258 counters of display_pixel.h,
// k_display_exposure turns them into an EV on the device (the adaptation state never leaves it), k_display_map multiplies by 2^EV,
// applies a tone operator and writes RGBA8.  The per-pixel code is display_pixel.h's, the functions spcbpt_display_host runs on the host.
// Integer atomics only: the histogram is the same on every run and for every grid size.
// (kernel_config.h maps the other kernel files)
#include <hip/hip_runtime.h>

#include "kernel_config.h"
#include "kernels_display.h"

namespace spc {

static constexpr int kDisplayWaves = BLOCK / 64;
static constexpr int kDisplayLoads = 4;             // float4 loads a lane has in flight per trip of the grid-stride loop
static constexpr int kDisplayHistBlocksMax = 1024;  // a few blocks per CU: a block folds pixels / 1024 of a large image into one flush

// Grid-stride over the pixels in index order, consecutive lanes on consecutive float4s.  Every wave counts into a sub-histogram of its
// own in LDS (258 words each, 4 128 B per block) with integer atomicAdd: lanes of one wave that meet in a bin serialise inside that
// ds_add, but one hot bin does not make the block's four waves queue behind each other.  One flush per block: thread b sums bin b over
// the waves (consecutive lanes on consecutive banks) and issues one global uint32 atomic add, skipping zeros.
__global__ __launch_bounds__(BLOCK) void k_display_histogram(const DisplayParams p) {
    __shared__ uint32_t s_hist[kDisplayWaves][kDisplayCounters];
    for (int b = threadIdx.x; b < kDisplayWaves * kDisplayCounters; b += BLOCK) (&s_hist[0][0])[b] = 0u;
    __syncthreads();
    uint32_t* mine = s_hist[threadIdx.x / 64];
    const size_t stride = (size_t)gridDim.x * BLOCK;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < p.pixels; i += stride * kDisplayLoads) {
        float4 v[kDisplayLoads];
#pragma unroll
        for (int k = 0; k < kDisplayLoads; k++) {
            const size_t j = i + (size_t)k * stride;
            if (j < p.pixels) v[k] = ldq(p.src, j);
        }
#pragma unroll
        for (int k = 0; k < kDisplayLoads; k++) {
            const size_t j = i + (size_t)k * stride;
            if (j < p.pixels) atomicAdd(&mine[display_bin(display_luminance(v[k].x, v[k].y, v[k].z))], 1u);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kDisplayCounters; b += BLOCK) {
        uint32_t n = 0;
#pragma unroll
        for (int w = 0; w < kDisplayWaves; w++) n += s_hist[w][b];
        if (n) atomicAdd(&p.state[b], n);
    }
}

// One wave; lane 0 runs display_auto_ev on the counters and leaves EV and "there is a previous EV" in the record.
__global__ __launch_bounds__(64) void k_display_exposure(const DisplayParams p) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool have_prev = p.state[kDisplayStateHavePrev] != 0u;
    const float prev = __uint_as_float(p.state[kDisplayStateEv]);
    const float ev = display_auto_ev(p.state, p.exposure, have_prev, prev);
    p.state[kDisplayStateEv] = __float_as_uint(ev);
    p.state[kDisplayStateHavePrev] = 1u;
}

// One lane per pixel in index order: a 16-byte load, a 4-byte store.  EV comes from the record (a uniform load) when auto is on.
__global__ __launch_bounds__(BLOCK) void k_display_map(const DisplayParams p) {
    const size_t idx = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (idx >= p.pixels) return;
    const float ev = p.auto_ev ? __uint_as_float(p.state[kDisplayStateEv]) : p.ev;
    const float4 v = ldq(p.src, idx);
    p.frame[idx] = display_tone(v.x, v.y, v.z, exp2f(ev), p.op, p.white);
}

void launch_display_histogram(const DisplayParams& p, hipStream_t s) {
    if (p.pixels == 0 || !p.src || !p.state) return;
    const size_t blocks = (p.pixels + BLOCK - 1) / BLOCK;
    const dim3 grid((unsigned)(blocks < (size_t)kDisplayHistBlocksMax ? blocks : (size_t)kDisplayHistBlocksMax));
    hipLaunchKernelGGL(k_display_histogram, grid, dim3(BLOCK), 0, s, p);
}

void launch_display_exposure(const DisplayParams& p, hipStream_t s) {
    if (!p.state) return;
    hipLaunchKernelGGL(k_display_exposure, dim3(1), dim3(64), 0, s, p);
}

void launch_display_map(const DisplayParams& p, hipStream_t s) {
    if (p.pixels == 0 || !p.src || !p.frame || (p.auto_ev && !p.state)) return;
    hipLaunchKernelGGL(k_display_map, dim3((unsigned)((p.pixels + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, p);
}

}  // namespace spc
