// The history reprojection (spcbpt_history_*): k_reproject carries a captured image into the current view through the first-hit
// depth and the two cameras (reproject_pixel.h, the function spcbpt_history_reproject_host runs on the host), k_resolve blends that
// prior with the film and tone-maps -- or, for a capture, writes the blend into the history plane.
// k_reproject_var / k_resolve_var are the forms that also carry the variance of what is shown (spcbpt_history_denoise).
// (kernel_config.h maps the other kernel files)
#include <hip/hip_runtime.h>

#include "device_lib.h"
#include "kernel_config.h"
#include "kernels_reproject.h"

namespace spc {

// One lane per pixel with the denoiser's mapping: a block is 32 x 8 pixels, a wave one 8 x 8 tile of it -- the four taps of a wave's
// pixels then fall into one compact patch of the history planes.  That patch is not block-aligned in the source (it moves with the
// camera), so there is no LDS stage: float4 loads, float4 stores, no atomics.
static constexpr int RP_BX = 32, RP_BY = 8;
SPC_DEV bool reproject_pixel_of_lane(uint32_t width, uint32_t height, int& x, int& y) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    x = (int)blockIdx.x * RP_BX + wave * 8 + (lane & 7);
    y = (int)blockIdx.y * RP_BY + (lane >> 3);
    return x < (int)width && y < (int)height;
}
static dim3 reproject_grid(uint32_t width, uint32_t height) { return dim3((width + RP_BX - 1) / RP_BX, (height + RP_BY - 1) / RP_BY); }

struct HistoryPlanes {   // reproject_pixel's F over the global float4 planes
    const float *g, *h;
    uint32_t width;
    SPC_DEV void fetch(int x, int y, float* G, float* H) const {
        const size_t i = (size_t)y * width + x;
        const float4 a = ldq(g, i), b = ldq(h, i);
        G[0] = a.x; G[1] = a.y; G[2] = a.z; G[3] = a.w;
        H[0] = b.x; H[1] = b.y; H[2] = b.z; H[3] = b.w;
    }
};

__global__ __launch_bounds__(BLOCK) void k_reproject(const ReprojectParams p) {
    int x, y;
    if (!reproject_pixel_of_lane(p.width, p.height, x, y)) return;
    const size_t idx = (size_t)y * p.width + x;
    const float4 nd = ldq(p.normal_depth, idx);
    const float nd4[4] = {nd.x, nd.y, nd.z, nd.w};
    const HistoryPlanes f = {p.hist_normal_depth, p.hist_rgbn, p.width};
    float out[4];
    reproject_pixel(f, p.cur, p.hist, (int)p.width, (int)p.height, x, y, nd4, p.step, out);
    reinterpret_cast<float4*>(p.prior)[idx] = make_float4(out[0], out[1], out[2], out[3]);
}

__global__ __launch_bounds__(BLOCK) void k_resolve(const ResolveParams p) {
    int x, y;
    if (!reproject_pixel_of_lane(p.width, p.height, x, y)) return;
    const size_t idx = (size_t)y * p.width + x;
    const float4 acc = ldq(p.accum, idx);
    const float a4[4] = {acc.x, acc.y, acc.z, acc.w};
    float out[4];
    if (p.prior) {   // (two calls, not one with a selected pointer: that would put the arrays into scratch)
        const float4 r = ldq(p.prior, idx);
        const float r4[4] = {r.x, r.y, r.z, r.w};
        resolve_pixel(r4, a4, p.frames, out);
    } else {
        resolve_pixel(nullptr, a4, p.frames, out);
    }
    reinterpret_cast<float4*>(p.out)[idx] = make_float4(out[0], out[1], out[2], out[3]);
    if (p.frame) p.frame[idx] = film_tone_map(mk3(out[0], out[1], out[2]));
}

// ---- the variance-carrying forms: what the two kernels above write, bit for bit, and the variance of it in a plane beside -----------
struct HistoryVarPlanes {   // reproject_var_pixel's F over the global float4 planes
    const float *g, *h, *hv;
    uint32_t width;
    SPC_DEV void fetch(int x, int y, float* G, float* H, float* HV) const {
        const size_t i = (size_t)y * width + x;
        const float4 a = ldq(g, i), b = ldq(h, i), c = ldq(hv, i);
        G[0] = a.x; G[1] = a.y; G[2] = a.z; G[3] = a.w;
        H[0] = b.x; H[1] = b.y; H[2] = b.z; H[3] = b.w;
        HV[0] = c.x; HV[1] = c.y; HV[2] = c.z; HV[3] = c.w;
    }
};

__global__ __launch_bounds__(BLOCK) void k_reproject_var(const ReprojectVarParams pv) {
    const ReprojectParams& p = pv.base;
    int x, y;
    if (!reproject_pixel_of_lane(p.width, p.height, x, y)) return;
    const size_t idx = (size_t)y * p.width + x;
    const float4 nd = ldq(p.normal_depth, idx);
    const float nd4[4] = {nd.x, nd.y, nd.z, nd.w};
    const HistoryVarPlanes f = {p.hist_normal_depth, p.hist_rgbn, pv.hist_var, p.width};
    float out[4], var[4];
    reproject_var_pixel(f, p.cur, p.hist, (int)p.width, (int)p.height, x, y, nd4, p.step, out, var);
    reinterpret_cast<float4*>(p.prior)[idx] = make_float4(out[0], out[1], out[2], out[3]);
    reinterpret_cast<float4*>(pv.prior_var)[idx] = make_float4(var[0], var[1], var[2], var[3]);
}

__global__ __launch_bounds__(BLOCK) void k_resolve_var(const ResolveVarParams pv) {
    const ResolveParams& p = pv.base;
    int x, y;
    if (!reproject_pixel_of_lane(p.width, p.height, x, y)) return;
    const size_t idx = (size_t)y * p.width + x;
    const float4 acc = ldq(p.accum, idx), mo = ldq(pv.m2n, idx);
    const float a4[4] = {acc.x, acc.y, acc.z, acc.w}, m4[4] = {mo.x, mo.y, mo.z, mo.w};
    float out[4], var[4];
    if (p.prior) {   // (two calls, as in k_resolve: selected pointers would put the arrays into scratch)
        const float4 r = ldq(p.prior, idx), rv = ldq(pv.prior_var, idx);
        const float r4[4] = {r.x, r.y, r.z, r.w}, rv4[4] = {rv.x, rv.y, rv.z, rv.w};
        resolve_var_pixel(r4, rv4, a4, m4, p.frames, out, var);
    } else {
        resolve_var_pixel(nullptr, nullptr, a4, m4, p.frames, out, var);
    }
    reinterpret_cast<float4*>(p.out)[idx] = make_float4(out[0], out[1], out[2], out[3]);
    reinterpret_cast<float4*>(pv.out_var)[idx] = make_float4(var[0], var[1], var[2], var[3]);
    if (p.frame) p.frame[idx] = film_tone_map(mk3(out[0], out[1], out[2]));
}

void launch_reproject(const ReprojectParams& p, hipStream_t s) {
    hipLaunchKernelGGL(k_reproject, reproject_grid(p.width, p.height), dim3(BLOCK), 0, s, p);
}
void launch_resolve(const ResolveParams& p, hipStream_t s) {
    hipLaunchKernelGGL(k_resolve, reproject_grid(p.width, p.height), dim3(BLOCK), 0, s, p);
}
void launch_reproject_var(const ReprojectVarParams& p, hipStream_t s) {
    hipLaunchKernelGGL(k_reproject_var, reproject_grid(p.base.width, p.base.height), dim3(BLOCK), 0, s, p);
}
void launch_resolve_var(const ResolveVarParams& p, hipStream_t s) {
    hipLaunchKernelGGL(k_resolve_var, reproject_grid(p.base.width, p.base.height), dim3(BLOCK), 0, s, p);
}

}  // namespace spc
