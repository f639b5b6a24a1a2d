// Context: the light-tracing launch "lt" (kernels_splat.hip), and the exported camera projection it shares with the kernel
// (part of the C ABI library: see capi_common.h for the map of its translation units)
#include "capi_common.h"
#include "dev_splat.h"
#include "kernels_splat.h"

using namespace spc;

namespace spc {

// spcbpt_launch(ctx, "lt", ...): the cache of the sampler set an eye launch would read (`eset`), splatted onto the rows of the band
// set and merged into the film as this subframe.  Stream and event discipline are launch_render's: the launch takes the next render
// stream, waits for the set's sampler build, and records sets[eset].render so that no later light pass rewrites the set under it.
// Event counters (spcbpt_enable_counters) are left untouched: the splat kernel charges none.
int Context::launch_splat(uint32_t frame, int r0, int r1, int rs) {
    int rc = film_ready();
    if (rc) return rc;
    if (kp.scene.env.valid) {
        error = "lt: not with an environment map: the directly seen sky is not sampled by this estimator, and the sky vertices of the cache "
                "(SPCBPT_LV_DIRECTION) have no position to project";
        return SPCBPT_ERR_STATE;
    }
    if (!have_sampler) { error = "lt needs a built sampler (\"light trace\" -> spcbpt_build_sampler)"; return SPCBPT_ERR_STATE; }
    if ((rc = begin_render(r0, r1, rs))) return rc;
    kp.subframe = frame;
    kp.result = d_result[rk];
    if (rstream != stream) HIP_TRY(this, sets[eset].sampler.wait_on(rstream));
    // the splat buffer of this render stream: allocated at the first "lt" launch after a resize, so that a context that never
    // launches "lt" keeps its footprint (spcbpt_resize has synchronised every stream before the size changed)
    const size_t px = (size_t)kp.width * kp.height;
    if (d_splat[rk].cap != px * 4) d_splat[rk].release();   // (not grow-only: a smaller film gets a smaller buffer)
    HIP_TRY(this, d_splat[rk].reserve(px * 4));
    const int capacity = (int)std::min<size_t>(lvc_capacity, 0x7fffffff);
    const int threads = splat_block_threads();
    const int blocks = splat_blocks(std::min(4 * std::max(1, num_cus), (capacity + threads - 1) / threads));
    rc = ensure_spill((size_t)blocks * (size_t)threads, true);
    if (rc) return rc;
    SplatParams sp;
    memset(&sp, 0, sizeof(sp));
    sp.scene = kp.scene;
    memcpy(sp.eye, kp.eye, 12); memcpy(sp.U, kp.U, 12); memcpy(sp.V, kp.V, 12); memcpy(sp.W, kp.W, 12);
    sp.width = kp.width; sp.height = kp.height; sp.subframe = kp.subframe;
    sp.row_begin = kp.row_begin; sp.row_end = kp.row_end; sp.row_step = kp.row_step;
    sp.lvc = sets[eset].lvc; sp.sampler_counts = sets[eset].counts; sp.capacity = capacity;
    sp.splat = d_splat[rk]; sp.result = kp.result;
    sp.spill = kp.spill; sp.spill_entries = kp.spill_entries; sp.diag = kp.diag;
    HIP_TRY(this, hipMemsetAsync(d_splat[rk], 0, px * 16, rstream));
    time_begin("lt", rstream);
    launch_lt_splat(sp, blocks, rstream);
    launch_lt_resolve(sp, rstream);
    time_end();
    HIP_TRY(this, hipGetLastError());
    rc = render_done(eset);
    return rc ? rc : finish_frame();
}

}  // namespace spc

extern "C" int spcbpt_camera_splat(const float eye[3], const float U[3], const float V[3], const float W[3], int width, int height,
                                   const float point[3], float* dx, float* dy, int* px, int* py, float* weight) {
    if (!eye || !U || !V || !W || !point || width < 1 || height < 1) return 0;
    float x, y, we;
    int ix, iy;
    if (!camera_splat(eye, U, V, W, width, height, point, x, y, ix, iy, we)) return 0;
    if (dx) *dx = x;
    if (dy) *dy = y;
    if (px) *px = ix;
    if (py) *py = iy;
    if (weight) *weight = we;
    return 1;
}
