// HIP kernels of the SPCBPT hot path for gfx950 (wave64).  One lane = one pixel-sample (eye pass) or one
// light-trace core (light pass); a wave covers an 8x8 pixel tile so primary rays stay coherent.
//   k_spcbpt      <- __raygen__SPCBPT + __closesthit__eyeSubpath(+_LightSource) + __miss__BDPTVertex +
//                    __closesthit__occlusion (raygen.cu:319-443, hit_program.cu:58-147, 246-340)  [megakernel]
//   k_light_trace <- __raygen__lightTrace + __closesthit__lightSubpath (raygen.cu:620-685, hit_program.cu:341-438)
//   k_pt          <- __raygen__pinhole + __closesthit__radiance/lightsource (raygen.cu:71-170, hit_program.cu:148-180, 439-552)
//   sampler build <- MyThrustOp::LVC_Process (cuda_thrust/device_thrust.cu:241-332), on device
#include <hip/hip_runtime.h>

#include "device_lib.h"
#include "dev_lens.h"
#include "eye_walk.h"
#include "job_order.h"
#include "kernel_config.h"
#include "kernels.h"
#include "kernels_adaptive.h"

namespace spc {

// The eye megakernel's block.  Its waves share nothing but the LDS copy of the hottest BVH nodes (s_hot below), and a CU holds 16 of
// them whatever the block size (4 per SIMD at 128 VGPRs; 16 x (4 KB of stack + a 5 840-B pool record) = 155 KB of its 160 KB of
// LDS): the larger the block, the fewer copies of that table share what is left -- 19 nodes in each of four 256-thread blocks, 38
// in each of two 512-thread blocks, 64 (all the builder numbers first) in ONE block of 1 024 threads per CU.
#ifndef SPC_EYE_BLOCK
#define SPC_EYE_BLOCK 256
#endif
// Issue priority of a wave by phase (s_setprio, 0 .. 3): see the traversal pass in k_spcbpt
#ifndef SPC_PRIO_TRAV
#define SPC_PRIO_TRAV 1
#endif
#ifndef SPC_PRIO_CONNECT
#define SPC_PRIO_CONNECT 0
#endif
#ifndef SPC_PRIO_SHADE
#define SPC_PRIO_SHADE 0
#endif
static constexpr int EYE_BLOCK = SPC_EYE_BLOCK;
static constexpr int EYE_HOT = SPC_EYE_BLOCK >= 1024 ? 64 : (SPC_EYE_BLOCK >= 512 ? 38 : 19);   // node records [0, EYE_HOT) live in LDS
// (carrying the pool's slot and pmf arrays in registers to make room for 96 more hot nodes: +0.9 %, profiles/r05_experiments.md, section 24)
static_assert(EYE_HOT <= HOT_NODES, "the builder numbers HOT_NODES nodes first (layout.h)");
static_assert(STACK_LDS >= 16, "the pooled connections publish 16 dwords per eye vertex through the traversal-stack LDS");
#ifndef SPC_EYE_WAVES
// ... and for the eye megakernel.  Measured on MI355X (bedroom 1080p, ms per frame).  With the pooled if-if traversal, one frame
// per launch: 2 (241 VGPR, no scratch) -> 12.86, 3 (168 VGPR, 252 B scratch) -> 10.72, 4 (128 VGPR, 452 B) -> 11.01,
// 5 (96 VGPR, 688 B) -> 14.16.  With pooled connections, immediate regeneration and batched launches the balance moved: the
// kernel is bound by the latency of dependent gathers (its throughput is 1 : 1.71 : 2.20 at 1, 2, 3 resident blocks per CU),
// and 4 (128 VGPR, 372 B scratch) gives 25.9 instead of 28.4 ms per 4-frame launch -- provided the block fits 4 times into
// the 160 KB of LDS, hence the 16-entry stack and the three eye-vertex dwords that travel by ds_bpermute instead (below).
#define SPC_EYE_WAVES 4
#endif

// The SPCBPT megakernel: persistent waves with per-lane path regeneration.  A wave pulls 8x8 pixel tiles from a global
// queue (one atomicAdd per tile); a lane whose eye path ends writes its pixel and immediately starts the next
// pixel-sample of the wave's pool, so the 64 lanes stay busy although path lengths differ by an order of magnitude.
// Every iteration runs the same phases for all live lanes: pooled traversal pass -> connections of the previous vertex ->
// new vertex + two-stage resampling.  The queue counter saturates, so every wave reaches the exit.
// Known cost: an eye path may live for 50 bounces (a dependent chain of milliseconds); once the queue is empty the waves drain
// their last paths with ever fewer live lanes -- measured with the wave clocks of the counting build, the average wave has
// left after 83 % of the kernel span.  Ordering the queue by the longest path each tile held in the previous frame did not
// shorten that (long paths are decided by Russian roulette, not by the pixel).
// BATCH: the tiles of p.n_frames frames (same camera and bands, each with its own sampler tables, subframe index and result
// buffer: p.frames) share one queue, so a wave keeps regenerating across frame boundaries and the drain phase is paid once per
// batch instead of once per frame -- what a rank's small share of a sharded frame needs.  Every pixel-sample is computed exactly
// as in a launch of its own frame; BATCH = false compiles to the single-frame kernel unchanged.
// CACHE: label caching (device_lib.h).  <false, *, true> are the timed kernels; <true, false, false> evaluates in the reference's
// order and charges its events (the contract's byte table, and the generic form for classifier trees with direction nodes);
// <true, false, true> counts the events the TIMED kernels execute (roofline.frac: what runs, not what the reference would run).
// ENV = false (timed forms only, chosen by the launcher for a scene with neither an environment map nor a material flagged
// `brdf`, DeviceScene::general == 0): the direction tests and the flag's divisions (device_lib.h brdf_div) are compiled out.
template <bool COUNT, bool BATCH, bool CACHE, bool ENV = true>
__global__ __launch_bounds__(EYE_BLOCK, SPC_EYE_WAVES) void k_spcbpt(const KParams p) {
    constexpr bool SKY = false;   // escaped eye paths end unseen (__miss__BDPTVertex), as upstream
    constexpr bool TILES = false, LENS = false;
#include "eye_kernel_body.h"
}
// SKY: the escaped eye paths see the environment map (eye_sky_miss; spcbpt_set_environment_mode, SPCBPT_ENV_EYE_SEES_SKY) -- the timed
// form of a scene with a sky (label caching, no counters), a kernel of its own so that the k_spcbpt forms keep their code
template <bool BATCH>
__global__ __launch_bounds__(EYE_BLOCK, SPC_EYE_WAVES) void k_spcbpt_sky(const KParams p) {
    constexpr bool COUNT = false, CACHE = true, ENV = true, SKY = true, TILES = false, LENS = false;
#include "eye_kernel_body.h"
}
// TILES: adaptive sampling (spcbpt_launch_adaptive).  The queue is p.tile_list[0 .. p.n_tiles) instead of a tile range, and the pixels of
// tile t draw sample p.tile_samples[t] instead of p.subframe: seed and jitter of camera_ray are those of an ordinary launch of that
// subframe, so every sample is bit for bit the uniform renderer's.  The timed single-frame form (label caching, no counters, results
// through film_write into p.result), a kernel of its own so that the k_spcbpt forms keep their code.
template <bool ENV>
__global__ __launch_bounds__(EYE_BLOCK, SPC_EYE_WAVES) void k_spcbpt_tiles(const KParams p) {
    constexpr bool COUNT = false, BATCH = false, CACHE = true, SKY = false, TILES = true, LENS = false;
#include "eye_kernel_body.h"
}
// LENS: the thin-lens camera (spcbpt_set_lens with a radius > 0; camera_lens.h).  Every pixel-sample starts at a lens point of its own
// (camera_ray_lens: two more random numbers behind the jitter's) and aims at the sample's point on the plane in focus; the rest of the
// walk is the pinhole form's.  The timed single-frame form (label caching, no counters), a kernel of its own so that the k_spcbpt forms
// keep their code: it alone carries the camera position in registers across the traversal pass (eye_kernel_body.h).
template <bool ENV>
__global__ __launch_bounds__(EYE_BLOCK, SPC_EYE_WAVES) void k_spcbpt_lens(const KParams p) {
    constexpr bool COUNT = false, BATCH = false, CACHE = true, SKY = false, TILES = false, LENS = true;
#include "eye_kernel_body.h"
}

// ------------------------------------------------------------------------------------------------
template <bool COUNT>
__global__ __launch_bounds__(BLOCK, SPC_WAVES) void k_pt(const KParams p) {
    constexpr bool LENS = false;
#include "pt_kernel_body.h"
}
// ... with the thin-lens camera (spcbpt_set_lens): the primary ray starts at a lens point.  The plain form only, and a kernel of its own
// name: the two k_pt<COUNT> instantiations keep their code and stay the only two (tests/test_codegen_mesh_light.py counts them).
__global__ __launch_bounds__(BLOCK, SPC_WAVES) void k_pt_lens(const KParams p) {
    constexpr bool COUNT = false, LENS = true;
#include "pt_kernel_body.h"
}

// ---- host-callable launchers ---------------------------------------------------------------------
static inline int render_blocks(const KParams& p) {
    const int tiles_x = ((int)p.width + 7) / 8;
    const int band_begin = p.row_begin / 8;
    const int band_end = (std::min(p.row_end, (int)p.height) + 7) / 8;
    const int step = p.row_step < 1 ? 1 : p.row_step;
    const int nb = band_end > band_begin ? (band_end - band_begin + step - 1) / step : 0;
    const int waves = tiles_x * nb;
    return (waves + (BLOCK / 64) - 1) / (BLOCK / 64);   // (k_pt, the film merges: one wave per tile, 256-thread blocks)
}
// threads of the widest grid a render launch of these bands may run ("pt": one wave per tile; "SPCBPT_eye": the same waves in the eye
// kernel's blocks) -- what the traversal stack's HBM area is sized for
int render_thread_count(const KParams& p) {
    const int waves = render_blocks(p) * (BLOCK / 64);
    return (waves + (EYE_BLOCK / 64) - 1) / (EYE_BLOCK / 64) * EYE_BLOCK;
}
int spcbpt_block_threads() { return EYE_BLOCK; }

// the escaped eye paths of this launch see the sky (spcbpt_set_environment_mode): the k_spcbpt_sky forms, timed variant only
// (the host refuses the counting variants then: Context::launch_render)
bool eye_sees_sky(const KParams& p) { return p.scene.env.valid && (p.scene.env.mode & SPCBPT_ENV_EYE_SEES_SKY) != 0; }
// variant: 0 = timed (label caching, no counters), 1 = reference order with counters (also the generic form), 2 = the timed
// kernel's own events, counted
void launch_spcbpt(const KParams& p, int variant, int max_blocks, hipStream_t s) {
    // persistent grid: at most `max_blocks` (resident) blocks, never more than the tile queue can feed
    const int tiles = (int)p.n_tiles;
    if (tiles <= 0) return;
    int blocks = (tiles + (EYE_BLOCK / 64) - 1) / (EYE_BLOCK / 64);
    if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
    if (variant == 1) {   // the reference's own evaluation of Gamma / Q (three reads, one division), counted as such
        KParams q = p;
        q.gamma_q = nullptr;
        hipLaunchKernelGGL((k_spcbpt<true, false, false>), dim3(blocks), dim3(EYE_BLOCK), 0, s, q);
    }
    else if (variant == 2) hipLaunchKernelGGL((k_spcbpt<true, false, true>), dim3(blocks), dim3(EYE_BLOCK), 0, s, p);
    else if (eye_sees_sky(p)) hipLaunchKernelGGL((k_spcbpt_sky<false>), dim3(blocks), dim3(EYE_BLOCK), 0, s, p);
    else if (p.scene.general) hipLaunchKernelGGL((k_spcbpt<false, false, true, true>), dim3(blocks), dim3(EYE_BLOCK), 0, s, p);
    else hipLaunchKernelGGL((k_spcbpt<false, false, true, false>), dim3(blocks), dim3(EYE_BLOCK), 0, s, p);
}
// p.frames / p.n_frames describe the batch; p.n_tiles is the tile count of ONE frame
int spcbpt_batch_blocks(const KParams& p, int max_blocks) {
    const long long tiles = (long long)p.n_tiles * p.n_frames;
    if (tiles <= 0) return 0;
    long long blocks = (tiles + (EYE_BLOCK / 64) - 1) / (EYE_BLOCK / 64);
    if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
    return (int)blocks;
}
void launch_spcbpt_batch(const KParams& p, int max_blocks, hipStream_t s) {
    const int blocks = spcbpt_batch_blocks(p, max_blocks);
    if (blocks <= 0) return;
    if (eye_sees_sky(p)) hipLaunchKernelGGL((k_spcbpt_sky<true>), dim3((unsigned)blocks), dim3(EYE_BLOCK), 0, s, p);
    else if (p.scene.general) hipLaunchKernelGGL((k_spcbpt<false, true, true, true>), dim3((unsigned)blocks), dim3(EYE_BLOCK), 0, s, p);
    else hipLaunchKernelGGL((k_spcbpt<false, true, true, false>), dim3((unsigned)blocks), dim3(EYE_BLOCK), 0, s, p);
}
// ... and of the list-fed form: p.n_tiles is the list's length, p.tile_list / p.tile_samples the list and the film's per-tile sample indices
int spcbpt_tiles_blocks(const KParams& p, int max_blocks) {
    const long long tiles = (long long)p.n_tiles;
    if (tiles <= 0) return 0;
    long long blocks = (tiles + (EYE_BLOCK / 64) - 1) / (EYE_BLOCK / 64);
    if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
    return (int)blocks;
}
void launch_spcbpt_tiles(const KParams& p, int max_blocks, hipStream_t s) {
    const int blocks = spcbpt_tiles_blocks(p, max_blocks);
    if (blocks <= 0 || !p.tile_list || !p.tile_samples) return;
    if (p.scene.general) hipLaunchKernelGGL((k_spcbpt_tiles<true>), dim3((unsigned)blocks), dim3(EYE_BLOCK), 0, s, p);
    else hipLaunchKernelGGL((k_spcbpt_tiles<false>), dim3((unsigned)blocks), dim3(EYE_BLOCK), 0, s, p);
}
// ... and of the thin-lens form (p.lens_radius > 0): the tile range of launch_spcbpt, timed variant only (the host refuses the others)
int spcbpt_lens_blocks(const KParams& p, int max_blocks) {
    const long long tiles = (long long)p.n_tiles;
    if (tiles <= 0) return 0;
    long long blocks = (tiles + (EYE_BLOCK / 64) - 1) / (EYE_BLOCK / 64);
    if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
    return (int)blocks;
}
void launch_spcbpt_lens(const KParams& p, int max_blocks, hipStream_t s) {
    const int blocks = spcbpt_lens_blocks(p, max_blocks);
    if (blocks <= 0) return;
    if (p.scene.general) hipLaunchKernelGGL((k_spcbpt_lens<true>), dim3((unsigned)blocks), dim3(EYE_BLOCK), 0, s, p);
    else hipLaunchKernelGGL((k_spcbpt_lens<false>), dim3((unsigned)blocks), dim3(EYE_BLOCK), 0, s, p);
}
int spcbpt_lens_blocks_per_cu(bool general) {
    int n = 0;
    const hipError_t e = general ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_spcbpt_lens<true>, EYE_BLOCK, 0)
                                 : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_spcbpt_lens<false>, EYE_BLOCK, 0);
    return e == hipSuccess && n > 0 ? n : 1;
}
int spcbpt_tiles_blocks_per_cu(bool general) {
    int n = 0;
    const hipError_t e = general ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_spcbpt_tiles<true>, EYE_BLOCK, 0)
                                 : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_spcbpt_tiles<false>, EYE_BLOCK, 0);
    return e == hipSuccess && n > 0 ? n : 1;
}
// resident blocks per CU of the instantiation launch_spcbpt / launch_spcbpt_batch will really launch for (variant, batch, general, sky):
// the forms differ in registers and scratch (the ENV = false form exists because of that), so each is asked for itself
int spcbpt_blocks_per_cu(int variant, bool batch, bool general, bool sky) {
    int n = 0;
    hipError_t e;
    if (variant == 0 && sky) e = batch ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_spcbpt_sky<true>, EYE_BLOCK, 0)
                                       : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_spcbpt_sky<false>, EYE_BLOCK, 0);
    else if (variant == 1) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_spcbpt<true, false, false>, EYE_BLOCK, 0);
    else if (variant == 2) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_spcbpt<true, false, true>, EYE_BLOCK, 0);
    else if (batch) e = general ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_spcbpt<false, true, true, true>, EYE_BLOCK, 0)
                                : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_spcbpt<false, true, true, false>, EYE_BLOCK, 0);
    else e = general ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_spcbpt<false, false, true, true>, EYE_BLOCK, 0)
                     : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_spcbpt<false, false, true, false>, EYE_BLOCK, 0);
    return e == hipSuccess && n > 0 ? n : 1;
}
int render_tile_count(const KParams& p) {
    const int tiles_x = ((int)p.width + 7) / 8;
    const int band_begin = p.row_begin / 8;
    const int band_end = (std::min(p.row_end, (int)p.height) + 7) / 8;
    const int step = p.row_step < 1 ? 1 : p.row_step;
    const int nb = band_end > band_begin ? (band_end - band_begin + step - 1) / step : 0;
    return tiles_x * nb;
}
// accumulate + tone-map (raygen.cu:421-442) of one subframe from the `result` buffer a render kernel filled, for the pixels of
// the selected bands.  Separate from the render kernels so that consecutive frames' render kernels may overlap.
__global__ __launch_bounds__(BLOCK) void k_film_merge(const KParams p, const float* __restrict__ result) {
    uint32_t x, y;
    if (!lane_pixel(p, x, y)) return;
    const float4 r = reinterpret_cast<const float4*>(result)[(size_t)y * p.width + x];
    film_write(p, x, y, mk3(r.x, r.y, r.z));  // p.result is null here: the direct path
}
// ... of the frames of a batched launch in one pass: per pixel the running mean takes the frames in order (the same operations as
// `frames` launches of k_film_merge), the tone map is that of the last one
__global__ __launch_bounds__(BLOCK) void k_film_merge_batch(const KParams p, const MergeBatch m, int frames) {
    uint32_t x, y;
    if (!lane_pixel(p, x, y)) return;
    const size_t idx = (size_t)y * p.width + x;
    float4* acc = reinterpret_cast<float4*>(p.accum);
    f3 c = mk3(0.0f);
    bool have = false;
    for (int k = 0; k < frames; k++) {
        const float4 r = reinterpret_cast<const float4*>(m.result[k])[idx];
        f3 v = mk3(r.x, r.y, r.z);
        if (m.subframe[k] > 0) {
            if (!have) { const float4 prev = acc[idx]; c = mk3(prev.x, prev.y, prev.z); }
            const float a = 1.0f / (float)(m.subframe[k] + 1);
            v = lerp3(c, v, a);
        }
        c = v; have = true;
    }
    acc[idx] = make_float4(c.x, c.y, c.z, 1.0f);
    if (p.frame) {
        const float lum = 0.3f * c.x + 0.6f * c.y + 0.1f * c.z;
        const float s = 1.0f / (1.0f + lum / 1.5f);
        const f3 t = c * s;
        p.frame[idx] = quant8(to_srgb(clampf(t.x, 0.f, 1.f))) | (quant8(to_srgb(clampf(t.y, 0.f, 1.f))) << 8) |
                       (quant8(to_srgb(clampf(t.z, 0.f, 1.f))) << 16) | (255u << 24);
    }
}
void launch_film_merge_batch(const KParams& p, const MergeBatch& m, int frames, hipStream_t s) {
    const int blocks = render_blocks(p);
    if (blocks <= 0 || frames <= 0) return;
    KParams q = p;
    q.result = nullptr;
    hipLaunchKernelGGL(k_film_merge_batch, dim3(blocks), dim3(BLOCK), 0, s, q, m, frames);
}
void launch_film_merge(const KParams& p, hipStream_t s) {
    const int blocks = render_blocks(p);
    if (blocks <= 0 || !p.result) return;
    KParams q = p;
    q.result = nullptr;
    hipLaunchKernelGGL(k_film_merge, dim3(blocks), dim3(BLOCK), 0, s, q, p.result);
}
void launch_pt(const KParams& p, bool count, hipStream_t s) {
    const int blocks = render_blocks(p);
    if (blocks <= 0) return;
    if (count) hipLaunchKernelGGL(k_pt<true>, dim3(blocks), dim3(BLOCK), 0, s, p);
    else hipLaunchKernelGGL(k_pt<false>, dim3(blocks), dim3(BLOCK), 0, s, p);
}
void launch_pt_lens(const KParams& p, hipStream_t s) {
    const int blocks = render_blocks(p);
    if (blocks <= 0) return;
    hipLaunchKernelGGL(k_pt_lens, dim3(blocks), dim3(BLOCK), 0, s, p);
}

}  // namespace spc
