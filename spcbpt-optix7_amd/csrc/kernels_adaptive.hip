// Adaptive sampling's image-space kernels: k_tile_error reduces the film error (moments_pixel.h: film_error_pixel) of every 8x8 tile
// to its mean, k_tile_select compacts the tiles that still need samples into an ascending list, and k_film_merge_tiles merges the
// samples of the listed tiles, each with its tile's own sample index: the operations of k_film_moments followed by k_film_merge, in
// their order.  (The eye megakernel fed from the list, k_spcbpt_tiles, stands in kernels.hip; kernel_config.h maps the other kernel files.)
#include <hip/hip_runtime.h>

#include "eye_walk.h"
#include "kernel_config.h"
#include "kernels_adaptive.h"

namespace spc {

// One wave per tile, four tiles per block, one lane per pixel of the tile.  The lanes' terms are added by a __shfl_down tree (the fixed
// order adaptive_pixel.h describes and the host form repeats); lane 0 writes the tile's mean and how many pixels it is the mean of.
__global__ __launch_bounds__(BLOCK) void k_tile_error(const float* __restrict__ accum, const float* __restrict__ m2n, uint32_t width, uint32_t height,
                                                      uint32_t n_tiles, float* __restrict__ tile_error, uint32_t* __restrict__ tile_known) {
    const uint32_t tile = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tile >= n_tiles) return;   // (the whole wave)
    uint32_t x, y;
    const bool inside = adaptive_tile_pixel(width, height, tile, lane, &x, &y);
    float c3[3] = {0.0f, 0.0f, 0.0f}, m4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (inside) {
        const size_t idx = (size_t)y * width + x;
        const float4 c = ldq(accum, idx), m = ldq(m2n, idx);
        c3[0] = c.x; c3[1] = c.y; c3[2] = c.z;
        m4[0] = m.x; m4[1] = m.y; m4[2] = m.z; m4[3] = m.w;
    }
    float e;
    uint32_t have;
    adaptive_slot_term(c3, m4, inside, &e, &have);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        e += __shfl_down(e, off, 64);
        have += __shfl_down(have, off, 64);
    }
    if (lane == 0) {
        tile_error[tile] = adaptive_tile_mean(e, have);
        tile_known[tile] = have;
    }
}
void launch_tile_error(const float* accum, const float* m2n, uint32_t width, uint32_t height, float* tile_error, uint32_t* tile_known, hipStream_t s) {
    const uint32_t n_tiles = adaptive_tiles_x(width) * adaptive_tiles_y(height);
    const uint32_t blocks = (n_tiles + (BLOCK / 64) - 1) / (BLOCK / 64);
    hipLaunchKernelGGL(k_tile_error, dim3(blocks), dim3(BLOCK), 0, s, accum, m2n, width, height, n_tiles, tile_error, tile_known);
}

// One block.  Thread i owns the tiles [i chunk, (i + 1) chunk): it counts the selected ones, the block scans the counts through LDS, and
// the thread writes its tiles behind those of the threads before it -- the list is ascending whatever the machine does.
static constexpr int SELECT_BLOCK = 1024;
__global__ __launch_bounds__(SELECT_BLOCK) void k_tile_select(const float* __restrict__ tile_error, const uint32_t* __restrict__ tile_known,
                                                              const uint32_t* __restrict__ tile_samples, uint32_t n_tiles, float target_error, uint32_t min_samples,
                                                              uint32_t max_samples, uint32_t* __restrict__ tiles, uint32_t* __restrict__ n_out) {
    __shared__ uint32_t s_scan[SELECT_BLOCK];
    const uint32_t chunk = (n_tiles + SELECT_BLOCK - 1) / SELECT_BLOCK;
    const uint32_t begin = min(threadIdx.x * chunk, n_tiles), end = min(begin + chunk, n_tiles);
    uint32_t mine = 0;
    for (uint32_t t = begin; t < end; t++)
        mine += adaptive_tile_selected(tile_samples[t], tile_error[t], tile_known[t] == 0u, target_error, min_samples, max_samples) ? 1u : 0u;
    s_scan[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t off = 1; off < SELECT_BLOCK; off <<= 1) {   // inclusive scan
        const uint32_t add = threadIdx.x >= off ? s_scan[threadIdx.x - off] : 0u;
        __syncthreads();
        s_scan[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t at = s_scan[threadIdx.x] - mine;
    for (uint32_t t = begin; t < end; t++)
        if (adaptive_tile_selected(tile_samples[t], tile_error[t], tile_known[t] == 0u, target_error, min_samples, max_samples)) tiles[at++] = t;
    if (threadIdx.x == SELECT_BLOCK - 1) *n_out = s_scan[SELECT_BLOCK - 1];
}
void launch_tile_select(const float* tile_error, const uint32_t* tile_known, const uint32_t* tile_samples, uint32_t n_tiles, float target_error,
                        uint32_t min_samples, uint32_t max_samples, uint32_t* tiles, uint32_t* n_out, hipStream_t s) {
    hipLaunchKernelGGL(k_tile_select, dim3(1), dim3(SELECT_BLOCK), 0, s, tile_error, tile_known, tile_samples, n_tiles, target_error, min_samples, max_samples,
                       tiles, n_out);
}

// One wave per LISTED tile, four per block, one pass.  With s = the tile's sample count: Welford's update of the moments from the mean
// before the merge (film_moments_update(., ., s): s == 0 restarts), then film_write's running mean with the weight 1 / (s + 1) and
// its tone map.  The count is written back by lane 0 after the wave's one load of it has returned (readfirstlane waits for it); no
// other wave touches the tile -- the list is strictly ascending.
__global__ __launch_bounds__(BLOCK) void k_film_merge_tiles(const MergeTilesParams p) {
    const uint32_t k = blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= p.n_listed) return;   // (the whole wave)
    const uint32_t tile = p.tile_list[k];
    const uint32_t samples = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.tile_samples[tile]);
    uint32_t x, y;
    if (adaptive_tile_pixel(p.width, p.height, tile, lane, &x, &y)) {
        const size_t idx = (size_t)y * p.width + x;
        const float4 r = ldq(p.result, idx);
        const float s3[3] = {r.x, r.y, r.z};
        float mean[3] = {0.0f, 0.0f, 0.0f}, m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (samples > 0) {
            const float4 a = ldq(p.accum, idx), b = ldq(p.m2n, idx);
            mean[0] = a.x; mean[1] = a.y; mean[2] = a.z;
            m[0] = b.x; m[1] = b.y; m[2] = b.z; m[3] = b.w;
        }
        film_moments_update(mean, s3, samples, m);
        reinterpret_cast<float4*>(p.m2n)[idx] = make_float4(m[0], m[1], m[2], m[3]);
        f3 c = mk3(r.x, r.y, r.z);
        if (samples > 0) {
            const float a = 1.0f / (float)(samples + 1);
            c = lerp3(mk3(mean[0], mean[1], mean[2]), c, a);
        }
        reinterpret_cast<float4*>(p.accum)[idx] = make_float4(c.x, c.y, c.z, 1.0f);
        if (p.frame) p.frame[idx] = film_tone_map(c);
    }
    if (lane == 0) p.tile_samples[tile] = samples + 1u;
}
void launch_film_merge_tiles(const MergeTilesParams& p, hipStream_t s) {
    if (p.n_listed == 0) return;
    hipLaunchKernelGGL(k_film_merge_tiles, dim3((p.n_listed + (BLOCK / 64) - 1) / (BLOCK / 64)), dim3(BLOCK), 0, s, p);
}

}  // namespace spc
