// The batched film merge that keeps the film's second moment and its buckets: k_film_merge_batch_stats is k_film_merge_batch (kernels.hip)
// with, per frame and in front of the mean's update, the operations of k_film_moments and k_film_buckets -- merge_stats_pixel.h, the
// function spcbpt_film_merge_batch_host runs on the host.  One launch stands for the 2 n or 3 n launches of n finish_frame calls.
// (kernel_config.h maps the other kernel files)
#include <hip/hip_runtime.h>

#include "eye_walk.h"
#include "kernel_config.h"
#include "kernels_merge_stats.h"

namespace spc {

// One lane per pixel, 8x8 tile per wave, four tiles per block: the launch shape of k_film_merge_batch (lane_pixel), so that exactly the
// pixels of the launch's bands are touched.  The lane owns its pixel for the whole batch: the mean and the second moment stay in
// registers (read once unless frame 0 overwrites them, written once), every frame's sample is read once, and the frame's bucket goes
// through memory -- a 16-byte load and store of entry subframe % K, of which this lane is the only writer, so program order is all the
// ordering a bucket that comes round again inside the batch needs.  No private array is indexed by the bucket: no scratch.
template <bool MOMENTS, bool BUCKETS>
__global__ __launch_bounds__(BLOCK) void k_film_merge_batch_stats(const MergeStatsParams p) {
    KParams q = {};
    q.width = p.width; q.height = p.height;
    q.row_begin = p.row_begin; q.row_end = p.row_end; q.row_step = p.row_step;
    uint32_t x, y;
    if (!lane_pixel(q, x, y)) return;
    const size_t px = (size_t)p.width * p.height, idx = (size_t)y * p.width + x;
    float4* acc = reinterpret_cast<float4*>(p.accum);
    float c[3] = {0.0f, 0.0f, 0.0f}, m[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (p.subframe[0] > 0) {   // (subframe 0 in front overwrites both)
        const float4 a = acc[idx];
        c[0] = a.x; c[1] = a.y; c[2] = a.z;
        if (MOMENTS) {
            const float4 b = ldq(p.m2n, idx);
            m[0] = b.x; m[1] = b.y; m[2] = b.z; m[3] = b.w;
        }
    }
    struct Entry {
        float4* at;   // the pixel in plane 0
        size_t px;
        SPC_DEV void load(int b, float* v) const { const float4 o = at[(size_t)b * px]; v[0] = o.x; v[1] = o.y; v[2] = o.z; v[3] = o.w; }
        SPC_DEV void store(int b, const float* v) const { at[(size_t)b * px] = make_float4(v[0], v[1], v[2], v[3]); }
    };
    const Entry entry = {reinterpret_cast<float4*>(p.planes) + idx, px};
    film_merge_stats_pixel<MOMENTS, BUCKETS>(
        p.frames, p.subframe,
        [&](int k, float* s) { const float4 r = ldq(p.result[k], idx); s[0] = r.x; s[1] = r.y; s[2] = r.z; },
        p.buckets, entry, c, m);
    acc[idx] = make_float4(c[0], c[1], c[2], 1.0f);
    if (MOMENTS) reinterpret_cast<float4*>(p.m2n)[idx] = make_float4(m[0], m[1], m[2], m[3]);
    if (p.frame) p.frame[idx] = film_tone_map(mk3(c[0], c[1], c[2]));   // film_write's tone map (device_lib.h), as k_film_merge_batch's
}

static int merge_stats_blocks(const MergeStatsParams& p) {
    // one wave per 8x8 tile of the selected bands, four tiles per block (render_blocks of kernels.hip)
    const int tiles_x = ((int)p.width + 7) / 8;
    const int band_begin = p.row_begin / 8;
    const int band_end = (std::min(p.row_end, (int)p.height) + 7) / 8;
    const int step = p.row_step < 1 ? 1 : p.row_step;
    const int nb = band_end > band_begin ? (band_end - band_begin + step - 1) / step : 0;
    return (tiles_x * nb + (BLOCK / 64) - 1) / (BLOCK / 64);
}
void launch_film_merge_batch_stats(const MergeStatsParams& p, hipStream_t s) {
    const int blocks = merge_stats_blocks(p);
    const bool moments = p.m2n != nullptr, buckets = p.buckets != 0;
    if (blocks <= 0 || !p.accum || p.frames < 1 || p.frames > kMergeStatsMaxFrames || (!moments && !buckets)) return;
    if (buckets && (!p.planes || !film_buckets_valid(p.buckets))) return;
    for (int k = 0; k < p.frames; k++)
        if (!p.result[k]) return;
    const dim3 grid((unsigned)blocks), block(BLOCK);
    if (moments && buckets) hipLaunchKernelGGL((k_film_merge_batch_stats<true, true>), grid, block, 0, s, p);
    else if (moments) hipLaunchKernelGGL((k_film_merge_batch_stats<true, false>), grid, block, 0, s, p);
    else hipLaunchKernelGGL((k_film_merge_batch_stats<false, true>), grid, block, 0, s, p);
}

}  // namespace spc
