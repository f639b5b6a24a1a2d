// Context + extern "C": the thin-lens camera (spcbpt_set_lens) -- its two numbers, the host forms of camera_lens.h, the random numbers a
// kernel draws for a pixel or a cache slot, and the debug kernel that writes the device's own lens rays
// (part of the C ABI library: see capi_common.h for the map of its translation units)
#include "capi_common.h"
#include "dev_lens.h"
#include "eye_walk.h"
#include "kernel_config.h"

using namespace spc;

namespace spc {

// One lane per pixel of the whole film (lane_pixel's 8x8 tiles): origin.xyz, direction.xyz, 0, 0 through camera_ray_lens -- the device
// function k_spcbpt_lens and k_pt_lens call.
__global__ __launch_bounds__(BLOCK) void k_debug_lens_rays(const KParams p, float* __restrict__ out) {
    uint32_t x, y;
    if (!lane_pixel(p, x, y)) return;
    uint32_t seed;
    f3 origin;
    const f3 dir = camera_ray_lens(p, x, y, seed, p.subframe, origin);
    float4* dst = reinterpret_cast<float4*>(out) + ((size_t)y * p.width + x) * 2;
    dst[0] = make_float4(origin.x, origin.y, origin.z, dir.x);
    dst[1] = make_float4(dir.y, dir.z, 0.0f, 0.0f);
}

int Context::set_lens(float radius, float focus) {
    if (!std::isfinite(radius) || !std::isfinite(focus)) { error = "set_lens: radius and focus must be finite"; return SPCBPT_ERR_INVALID_ARG; }
    if (radius < 0.0f) { error = "set_lens: the lens radius must be >= 0 (0 = the pinhole)"; return SPCBPT_ERR_INVALID_ARG; }
    if (!(focus > 0.0f)) { error = "set_lens: the focus depth must be > 0 (in units of W: 1 = the plane through lookat)"; return SPCBPT_ERR_INVALID_ARG; }
    // (launches already queued took their parameter block by value: nothing to wait for)
    kp.lens_radius = radius; kp.lens_focus = focus;
    update_lens_axes();
    return SPCBPT_OK;
}
// kp.lens_u / lens_v follow the camera and the radius (spcbpt_set_camera, spcbpt_set_lens); zero without a lens or a camera
void Context::update_lens_axes() {
    memset(kp.lens_u, 0, 12); memset(kp.lens_v, 0, 12);
    if (have_camera && kp.lens_radius > 0.0f) camera_lens_axes(kp.U, kp.V, kp.lens_radius, kp.lens_u, kp.lens_v);
}

int Context::debug_lens_rays(uint32_t subframe, float* out8) {
    if (!out8) { error = "debug_lens_rays: null pointer"; return SPCBPT_ERR_INVALID_ARG; }
    if (!d_accum) { error = "debug_lens_rays before spcbpt_resize"; return SPCBPT_ERR_STATE; }
    if (!have_camera) { error = "debug_lens_rays before spcbpt_set_camera"; return SPCBPT_ERR_STATE; }
    const size_t px = (size_t)kp.width * kp.height;
    DevBuf<float> d_out;
    HIP_TRY(this, d_out.reserve(px * 8));
    KParams q = kp;
    q.subframe = subframe; q.row_begin = 0; q.row_end = (int)kp.height; q.row_step = 1;
    const int tiles = (((int)kp.width + 7) / 8) * (((int)kp.height + 7) / 8);
    const int blocks = (tiles + (BLOCK / 64) - 1) / (BLOCK / 64);
    hipLaunchKernelGGL(k_debug_lens_rays, dim3((unsigned)blocks), dim3(BLOCK), 0, stream, q, d_out.p);
    HIP_TRY(this, hipGetLastError());
    HIP_TRY(this, hipStreamSynchronize(stream));
    HIP_TRY(this, hipMemcpy(out8, d_out.p, px * 8 * sizeof(float), hipMemcpyDeviceToHost));
    return SPCBPT_OK;
}

// tea4 and rnd of device_lib.h (../cuda/random.h:31-67) on the host: the stream a kernel draws a pixel's or a slot's numbers from
static uint32_t host_tea4(uint32_t v0, uint32_t v1) {
    uint32_t s0 = 0;
    for (int n = 0; n < 4; n++) {
        s0 += 0x9e3779b9u;
        v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4u);
        v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761eu);
    }
    return v0;
}
static float host_rnd(uint32_t& s) {
    s = 1664525u * s + 1013904223u;
    return (float)(s & 0x00FFFFFFu) / (float)0x01000000;
}

}  // namespace spc

extern "C" int spcbpt_set_lens(spcbpt_ctx* c, float radius, float focus) {
    CTX_CHECK(c);
    return c->set_lens(radius, focus);
}
extern "C" int spcbpt_get_lens(spcbpt_ctx* c, float* radius, float* focus) {
    CTX_CHECK(c);
    if (radius) *radius = c->kp.lens_radius;
    if (focus) *focus = c->kp.lens_focus;
    return SPCBPT_OK;
}
extern "C" int spcbpt_debug_lens_rays(spcbpt_ctx* c, uint32_t subframe, float* out8) {
    CTX_CHECK(c);
    return c->debug_lens_rays(subframe, out8);
}

extern "C" int spcbpt_lens_sample_host(uint32_t index, uint32_t subframe, int with_jitter, float out[4]) {
    if (!out) return SPCBPT_ERR_INVALID_ARG;
    uint32_t seed = host_tea4(index, subframe);
    out[0] = out[1] = 0.5f;
    if (with_jitter && subframe != 0) { out[0] = host_rnd(seed); out[1] = host_rnd(seed); }
    out[2] = host_rnd(seed);
    out[3] = host_rnd(seed);
    return SPCBPT_OK;
}

extern "C" int spcbpt_camera_lens_ray_host(const float eye[3], const float U[3], const float V[3], const float W[3], int width, int height, int n,
                                           const int32_t* xy, const float* jitter, const float* lens, float radius, float focus,
                                           float* origin, float* dir) {
    if (!eye || !U || !V || !W || width < 1 || height < 1 || n < 0) return SPCBPT_ERR_INVALID_ARG;
    if (n > 0 && (!xy || !jitter || !lens || !origin || !dir)) return SPCBPT_ERR_INVALID_ARG;
    if (!std::isfinite(radius) || !std::isfinite(focus) || radius < 0.0f || !(focus > 0.0f)) return SPCBPT_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++)
        camera_lens_ray(eye, U, V, W, width, height, xy[2 * i], xy[2 * i + 1], jitter[2 * i], jitter[2 * i + 1], lens[2 * i], lens[2 * i + 1], radius, focus,
                        origin + 3 * (size_t)i, dir + 3 * (size_t)i);
    return SPCBPT_OK;
}

extern "C" int spcbpt_camera_splat_lens(const float eye[3], const float U[3], const float V[3], const float W[3], int width, int height, int n,
                                        const float* points, const float* lens, float radius, float focus,
                                        float* dxdy, int32_t* pixel, float* weight, int32_t* inside) {
    if (!eye || !U || !V || !W || width < 1 || height < 1 || n < 0) return SPCBPT_ERR_INVALID_ARG;
    if (n > 0 && (!points || !lens || !inside)) return SPCBPT_ERR_INVALID_ARG;
    if (!std::isfinite(radius) || !std::isfinite(focus) || radius < 0.0f || !(focus > 0.0f)) return SPCBPT_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++) {
        float x = 0.0f, y = 0.0f, we = 0.0f;
        int ix = -1, iy = -1;
        const bool ok = camera_splat_lens(eye, U, V, W, width, height, points + 3 * (size_t)i, lens[2 * i], lens[2 * i + 1], radius, focus, x, y, ix, iy, we);
        inside[i] = ok ? 1 : 0;
        if (dxdy) { dxdy[2 * i] = ok ? x : 0.0f; dxdy[2 * i + 1] = ok ? y : 0.0f; }
        if (pixel) { pixel[2 * i] = ok ? ix : -1; pixel[2 * i + 1] = ok ? iy : -1; }
        if (weight) weight[i] = ok ? we : 0.0f;
    }
    return SPCBPT_OK;
}
