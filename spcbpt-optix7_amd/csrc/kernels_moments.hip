// The film's per-pixel second moment and the error estimate built on it: k_film_moments runs in front of a film merge and applies
// Welford's update (moments_pixel.h, the function spcbpt_film_moments_update_host runs on the host) to the pixels the merge is about to
// rewrite; k_film_error + k_film_error_final reduce the relative standard error of the film's pixels to (count, mean, maximum).
// (kernel_config.h maps the other kernel files)
#include <hip/hip_runtime.h>

#include "eye_walk.h"
#include "kernel_config.h"
#include "kernels_moments.h"

namespace spc {

// One lane per pixel, 8x8 tile per wave, four tiles per block: the launch shape of k_film_merge (lane_pixel), so that exactly the
// pixels of the launch's bands are touched.
__global__ __launch_bounds__(BLOCK) void k_film_moments(const MomentsParams p) {
    KParams q = {};
    q.width = p.width; q.height = p.height;
    q.row_begin = p.row_begin; q.row_end = p.row_end; q.row_step = p.row_step;
    uint32_t x, y;
    if (!lane_pixel(q, x, y)) return;
    const size_t idx = (size_t)y * p.width + x;
    const float4 r = ldq(p.result, idx);
    const float s3[3] = {r.x, r.y, r.z};
    float mean[3] = {0.0f, 0.0f, 0.0f}, m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (p.subframe > 0) {
        const float4 a = ldq(p.accum, idx), b = ldq(p.m2n, idx);
        mean[0] = a.x; mean[1] = a.y; mean[2] = a.z;
        m[0] = b.x; m[1] = b.y; m[2] = b.z; m[3] = b.w;
    }
    film_moments_update(mean, s3, p.subframe, m);
    reinterpret_cast<float4*>(p.m2n)[idx] = make_float4(m[0], m[1], m[2], m[3]);
}

static int moments_blocks(const MomentsParams& p) {
    // one wave per 8x8 tile of the selected bands, four tiles per block (render_blocks of kernels.hip)
    const int tiles_x = ((int)p.width + 7) / 8;
    const int band_begin = p.row_begin / 8;
    const int band_end = (std::min(p.row_end, (int)p.height) + 7) / 8;
    const int step = p.row_step < 1 ? 1 : p.row_step;
    const int nb = band_end > band_begin ? (band_end - band_begin + step - 1) / step : 0;
    return (tiles_x * nb + (BLOCK / 64) - 1) / (BLOCK / 64);
}
void launch_film_moments(const MomentsParams& p, hipStream_t s) {
    const int blocks = moments_blocks(p);
    if (blocks <= 0 || !p.result) return;
    hipLaunchKernelGGL(k_film_moments, dim3((unsigned)blocks), dim3(BLOCK), 0, s, p);
}

// ---- film error ---------------------------------------------------------------------------------
// (sum, maximum, count) of a block's lanes: every wave by shuffles in a fixed tree, the block's four waves through LDS in wave order.
// The result is valid in thread 0.
struct ErrAcc { double sum; float max; uint32_t count; };
SPC_DEV ErrAcc block_reduce(ErrAcc a, double* s_sum, float* s_max, uint32_t* s_count) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a.sum += __shfl_down(a.sum, off, 64);
        a.max = fmaxf(a.max, __shfl_down(a.max, off, 64));
        a.count += __shfl_down(a.count, off, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_sum[wave] = a.sum; s_max[wave] = a.max; s_count[wave] = a.count; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a.sum = s_sum[0]; a.max = s_max[0]; a.count = s_count[0];
        for (int w = 1; w < BLOCK / 64; w++) { a.sum += s_sum[w]; a.max = fmaxf(a.max, s_max[w]); a.count += s_count[w]; }
    }
    return a;
}

// Pixel i of the film goes to lane i % (blocks x BLOCK), whatever the machine: a lane adds its pixels' float32 terms in double, in
// index order.
__global__ __launch_bounds__(BLOCK) void k_film_error(const float* __restrict__ accum, const float* __restrict__ m2n, size_t pixels,
                                                      FilmErrorPartial* __restrict__ partials) {
    __shared__ double s_sum[BLOCK / 64];
    __shared__ float s_max[BLOCK / 64];
    __shared__ uint32_t s_count[BLOCK / 64];
    ErrAcc a = {0.0, 0.0f, 0u};
    const size_t stride = (size_t)gridDim.x * BLOCK;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < pixels; i += stride) {
        const float4 c = ldq(accum, i), m = ldq(m2n, i);
        const float c3[3] = {c.x, c.y, c.z}, m4[4] = {m.x, m.y, m.z, m.w};
        float e;
        if (film_error_pixel(c3, m4, &e)) { a.sum += (double)e; a.max = fmaxf(a.max, e); a.count += 1u; }
    }
    a = block_reduce(a, s_sum, s_max, s_count);
    if (threadIdx.x == 0) {
        FilmErrorPartial o;
        o.sum = a.sum; o.max = a.max; o.count = a.count;
        partials[blockIdx.x] = o;
    }
}
// One block: lane t adds partials t, t + BLOCK, ... in index order, then the same tree.  `out` is spcbpt_film_error_stats.
struct FilmErrorOut { long long pixels; double mean, max; };
__global__ __launch_bounds__(BLOCK) void k_film_error_final(const FilmErrorPartial* __restrict__ partials, int n, FilmErrorOut* __restrict__ out) {
    __shared__ double s_sum[BLOCK / 64];
    __shared__ float s_max[BLOCK / 64];
    __shared__ uint32_t s_count[BLOCK / 64];
    ErrAcc a = {0.0, 0.0f, 0u};
    for (int i = threadIdx.x; i < n; i += BLOCK) {
        const FilmErrorPartial q = partials[i];
        a.sum += q.sum; a.max = fmaxf(a.max, q.max); a.count += q.count;
    }
    a = block_reduce(a, s_sum, s_max, s_count);
    if (threadIdx.x == 0) {
        FilmErrorOut o;
        o.pixels = (long long)a.count;
        o.mean = a.count ? a.sum / (double)a.count : 0.0;
        o.max = a.count ? (double)a.max : 0.0;
        *out = o;
    }
}

int film_error_blocks(size_t pixels) {
    const size_t b = (pixels + BLOCK - 1) / BLOCK;
    return (int)std::min<size_t>(std::max<size_t>(b, 1), (size_t)kFilmErrorMaxBlocks);
}
void launch_film_error(const float* accum, const float* m2n, size_t pixels, FilmErrorPartial* partials, void* out, hipStream_t s) {
    const int blocks = film_error_blocks(pixels);
    hipLaunchKernelGGL(k_film_error, dim3((unsigned)blocks), dim3(BLOCK), 0, s, accum, m2n, pixels, partials);
    hipLaunchKernelGGL(k_film_error_final, dim3(1), dim3(BLOCK), 0, s, (const FilmErrorPartial*)partials, blocks, reinterpret_cast<FilmErrorOut*>(out));
}

}  // namespace spc
