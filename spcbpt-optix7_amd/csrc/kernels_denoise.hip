// The edge-avoiding a-trous denoiser on the demodulated film (spcbpt_denoise): k_demodulate divides the film by the first-hit albedo
// and turns depth into a position, k_atrous runs one iteration of the filter (denoise_pixel.h, the function spcbpt_denoise_host
// runs on the host) from one float4 plane into the other, k_remodulate multiplies the albedo back and tone-maps.
// k_demodulate_var / k_atrous_var / k_atrous_var_lds are the variance-guided form (spcbpt_denoise_variance) between the same planes;
// k_demodulate_resolved starts that form from the resolved image of the history reprojection (spcbpt_history_denoise).
// (kernel_config.h maps the other kernel files)
#include <hip/hip_runtime.h>

#include "device_lib.h"
#include "kernel_config.h"
#include "kernels_denoise.h"

namespace spc {

// One lane per pixel; a block is 32 x 8 pixels, a wave one 8 x 8 tile of it (eight lanes read 128 contiguous bytes of a row).
static constexpr int DN_BX = 32, DN_BY = 8;
SPC_DEV bool denoise_pixel_of_lane(const DenoiseParams& p, int& x, int& y) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    x = (int)blockIdx.x * DN_BX + wave * 8 + (lane & 7);
    y = (int)blockIdx.y * DN_BY + (lane >> 3);
    return x < (int)p.width && y < (int)p.height;
}
static dim3 denoise_grid(const DenoiseParams& p) { return dim3((p.width + DN_BX - 1) / DN_BX, (p.height + DN_BY - 1) / DN_BY); }

__global__ __launch_bounds__(BLOCK) void k_demodulate(const DenoiseParams p) {
    int x, y;
    if (!denoise_pixel_of_lane(p, x, y)) return;
    const size_t idx = (size_t)y * p.width + x;
    const float4 acc = ldq(p.accum, idx), alb = ldq(p.albedo, idx), nd = ldq(p.normal_depth, idx);
    const float a3[3] = {acc.x, acc.y, acc.z}, b3[3] = {alb.x, alb.y, alb.z};
    float c[3], X[3];
    denoise_demodulate(a3, b3, c);
    denoise_position(p.U, p.V, p.W, (int)p.width, (int)p.height, x, y, nd.w, X);
    reinterpret_cast<float4*>(p.ping)[idx] = make_float4(c[0], c[1], c[2], 0.0f);
    reinterpret_cast<float4*>(p.position)[idx] = make_float4(X[0], X[1], X[2], 0.0f);
}

struct GlobalPlanes {   // atrous_pixel's F over the global float4 planes
    const float *c, *n, *X;
    uint32_t width;
    SPC_DEV void fetch(int x, int y, float* cq, float* nq, float* Xq) const {
        const size_t i = (size_t)y * width + x;
        const float4 a = ldq(c, i), b = ldq(n, i), d = ldq(X, i);
        cq[0] = a.x; cq[1] = a.y; cq[2] = a.z;
        nq[0] = b.x; nq[1] = b.y; nq[2] = b.z;
        Xq[0] = d.x; Xq[1] = d.y; Xq[2] = d.z;
    }
};

__global__ __launch_bounds__(BLOCK) void k_atrous(const DenoiseParams p, const AtrousStep a, const float* __restrict__ src, float* __restrict__ dst) {
    int x, y;
    if (!denoise_pixel_of_lane(p, x, y)) return;
    const GlobalPlanes f = {src, p.normal_depth, p.position, p.width};
    float out[3];
    atrous_pixel(f, x, y, (int)p.width, (int)p.height, a, out);
    reinterpret_cast<float4*>(dst)[(size_t)y * p.width + x] = make_float4(out[0], out[1], out[2], 0.0f);
}

// Steps 1 and 2 (the plain-load k_atrous above serves the later ones): the 25 taps of a block's pixels fall into the block's tile plus a halo of 2 s pixels, and every input is read by up
// to 25 lanes of the block -- so the tile + halo of c, n and X is staged in LDS once (nine float planes of 40 x 16 entries, 23 KB: six
// blocks per CU) and the taps read LDS.  The row pitch of 40 puts the eight rows of a wave's 8 x 8 tile into eight disjoint groups
// of eight banks.  Pixels outside the image are not staged: atrous_pixel never asks for them.
static constexpr int DN_PITCH = DN_BX + 8, DN_ROWS = DN_BY + 8;
struct LdsPlanes {   // atrous_pixel's F over the staged tile
    const float* t;   // nine planes of DN_PITCH * DN_ROWS floats
    int x0, y0;       // image coordinates of entry (0, 0)
    SPC_DEV void fetch(int x, int y, float* cq, float* nq, float* Xq) const {
        const float* e = t + (y - y0) * DN_PITCH + (x - x0);
#pragma unroll
        for (int k = 0; k < 3; k++) {
            cq[k] = e[k * DN_PITCH * DN_ROWS];
            nq[k] = e[(3 + k) * DN_PITCH * DN_ROWS];
            Xq[k] = e[(6 + k) * DN_PITCH * DN_ROWS];
        }
    }
};
__global__ __launch_bounds__(BLOCK) void k_atrous_lds(const DenoiseParams p, const AtrousStep a, const float* __restrict__ src, float* __restrict__ dst) {
    __shared__ float s_tile[9 * DN_PITCH * DN_ROWS];
    const int halo = 2 * a.step;                                  // <= 4: launch_atrous sends steps 1 and 2 here
    const int x0 = (int)blockIdx.x * DN_BX - halo, y0 = (int)blockIdx.y * DN_BY - halo;
    const int cols = DN_BX + 2 * halo, rows = DN_BY + 2 * halo;   // <= DN_PITCH, DN_ROWS
    for (int i = threadIdx.x; i < cols * rows; i += BLOCK) {
        const int ty = i / cols, tx = i - ty * cols;
        const int gx = x0 + tx, gy = y0 + ty;
        if (gx < 0 || gy < 0 || gx >= (int)p.width || gy >= (int)p.height) continue;
        const size_t g = (size_t)gy * p.width + gx;
        const float4 c = ldq(src, g), n = ldq(p.normal_depth, g), X = ldq(p.position, g);
        float* e = s_tile + ty * DN_PITCH + tx;
        e[0] = c.x; e[DN_PITCH * DN_ROWS] = c.y; e[2 * DN_PITCH * DN_ROWS] = c.z;
        e[3 * DN_PITCH * DN_ROWS] = n.x; e[4 * DN_PITCH * DN_ROWS] = n.y; e[5 * DN_PITCH * DN_ROWS] = n.z;
        e[6 * DN_PITCH * DN_ROWS] = X.x; e[7 * DN_PITCH * DN_ROWS] = X.y; e[8 * DN_PITCH * DN_ROWS] = X.z;
    }
    __syncthreads();
    int x, y;
    if (!denoise_pixel_of_lane(p, x, y)) return;
    const LdsPlanes f = {s_tile, x0, y0};
    float out[3];
    atrous_pixel(f, x, y, (int)p.width, (int)p.height, a, out);
    reinterpret_cast<float4*>(dst)[(size_t)y * p.width + x] = make_float4(out[0], out[1], out[2], 0.0f);
}

// ---- the variance-guided form (spcbpt_denoise_variance): the same planes, with the variance of the demodulated luminance in .w ----
__global__ __launch_bounds__(BLOCK) void k_demodulate_var(const DenoiseParams p, const float* __restrict__ m2n) {
    int x, y;
    if (!denoise_pixel_of_lane(p, x, y)) return;
    const size_t idx = (size_t)y * p.width + x;
    const float4 acc = ldq(p.accum, idx), alb = ldq(p.albedo, idx), nd = ldq(p.normal_depth, idx), mo = ldq(m2n, idx);
    const float a3[3] = {acc.x, acc.y, acc.z}, b3[3] = {alb.x, alb.y, alb.z}, m4[4] = {mo.x, mo.y, mo.z, mo.w};
    float c[3], X[3];
    denoise_demodulate(a3, b3, c);
    denoise_position(p.U, p.V, p.W, (int)p.width, (int)p.height, x, y, nd.w, X);
    reinterpret_cast<float4*>(p.ping)[idx] = make_float4(c[0], c[1], c[2], denoise_variance_start(c, b3, m4));
    reinterpret_cast<float4*>(p.position)[idx] = make_float4(X[0], X[1], X[2], 0.0f);
}

// spcbpt_history_denoise: the start planes from the resolved image (p.accum) and its per-channel variance RV instead of film and moments
__global__ __launch_bounds__(BLOCK) void k_demodulate_resolved(const DenoiseParams p, const float* __restrict__ resolved_var) {
    int x, y;
    if (!denoise_pixel_of_lane(p, x, y)) return;
    const size_t idx = (size_t)y * p.width + x;
    const float4 res = ldq(p.accum, idx), alb = ldq(p.albedo, idx), nd = ldq(p.normal_depth, idx), rv = ldq(resolved_var, idx);
    const float a3[3] = {res.x, res.y, res.z}, b3[3] = {alb.x, alb.y, alb.z}, v3[3] = {rv.x, rv.y, rv.z};
    float c[3], X[3];
    denoise_demodulate(a3, b3, c);
    denoise_position(p.U, p.V, p.W, (int)p.width, (int)p.height, x, y, nd.w, X);
    reinterpret_cast<float4*>(p.ping)[idx] = make_float4(c[0], c[1], c[2], denoise_resolved_start(b3, v3));
    reinterpret_cast<float4*>(p.position)[idx] = make_float4(X[0], X[1], X[2], 0.0f);
}

struct GlobalVarPlanes : GlobalPlanes {   // atrous_var_pixel's F over the global float4 planes: v is c's .w
    SPC_DEV float variance(int x, int y) const { return c[((size_t)y * width + x) * 4 + 3]; }
};
__global__ __launch_bounds__(BLOCK) void k_atrous_var(const DenoiseParams p, const AtrousVarStep a, const float* __restrict__ src, float* __restrict__ dst) {
    int x, y;
    if (!denoise_pixel_of_lane(p, x, y)) return;
    GlobalVarPlanes f;
    f.c = src; f.n = p.normal_depth; f.X = p.position; f.width = p.width;
    float out[4];
    atrous_var_pixel(f, x, y, (int)p.width, (int)p.height, a, out);
    reinterpret_cast<float4*>(dst)[(size_t)y * p.width + x] = make_float4(out[0], out[1], out[2], out[3]);
}

// Steps 1 and 2 from LDS, like k_atrous_lds: ten planes (c, n, X and v) of 40 x 16 entries, 25.6 KB.  The 3 x 3 prefilter reads v at
// distance 1 of the block's OWN pixels only (v~ is taken at p, not at the taps), so the halo of 2 s >= 2 holds it.
struct LdsVarPlanes : LdsPlanes {
    SPC_DEV float variance(int x, int y) const { return t[9 * DN_PITCH * DN_ROWS + (y - y0) * DN_PITCH + (x - x0)]; }
};
__global__ __launch_bounds__(BLOCK) void k_atrous_var_lds(const DenoiseParams p, const AtrousVarStep a, const float* __restrict__ src, float* __restrict__ dst) {
    __shared__ float s_tile[10 * DN_PITCH * DN_ROWS];
    const int halo = 2 * a.step;                                  // 2 or 4: launch_atrous_var sends steps 1 and 2 here
    const int x0 = (int)blockIdx.x * DN_BX - halo, y0 = (int)blockIdx.y * DN_BY - halo;
    const int cols = DN_BX + 2 * halo, rows = DN_BY + 2 * halo;   // <= DN_PITCH, DN_ROWS
    for (int i = threadIdx.x; i < cols * rows; i += BLOCK) {
        const int ty = i / cols, tx = i - ty * cols;
        const int gx = x0 + tx, gy = y0 + ty;
        if (gx < 0 || gy < 0 || gx >= (int)p.width || gy >= (int)p.height) continue;
        const size_t g = (size_t)gy * p.width + gx;
        const float4 c = ldq(src, g), n = ldq(p.normal_depth, g), X = ldq(p.position, g);
        float* e = s_tile + ty * DN_PITCH + tx;
        e[0] = c.x; e[DN_PITCH * DN_ROWS] = c.y; e[2 * DN_PITCH * DN_ROWS] = c.z;
        e[3 * DN_PITCH * DN_ROWS] = n.x; e[4 * DN_PITCH * DN_ROWS] = n.y; e[5 * DN_PITCH * DN_ROWS] = n.z;
        e[6 * DN_PITCH * DN_ROWS] = X.x; e[7 * DN_PITCH * DN_ROWS] = X.y; e[8 * DN_PITCH * DN_ROWS] = X.z;
        e[9 * DN_PITCH * DN_ROWS] = c.w;
    }
    __syncthreads();
    int x, y;
    if (!denoise_pixel_of_lane(p, x, y)) return;
    LdsVarPlanes f;
    f.t = s_tile; f.x0 = x0; f.y0 = y0;
    float out[4];
    atrous_var_pixel(f, x, y, (int)p.width, (int)p.height, a, out);
    reinterpret_cast<float4*>(dst)[(size_t)y * p.width + x] = make_float4(out[0], out[1], out[2], out[3]);
}

__global__ __launch_bounds__(BLOCK) void k_remodulate(const DenoiseParams p, const float* __restrict__ src) {
    int x, y;
    if (!denoise_pixel_of_lane(p, x, y)) return;
    const size_t idx = (size_t)y * p.width + x;
    const float4 cl = ldq(src, idx), alb = ldq(p.albedo, idx);
    const float c3[3] = {cl.x, cl.y, cl.z}, b3[3] = {alb.x, alb.y, alb.z};
    float o[3];
    denoise_remodulate(c3, b3, o);
    reinterpret_cast<float4*>(p.denoised)[idx] = make_float4(o[0], o[1], o[2], 1.0f);
    p.frame[idx] = film_tone_map(mk3(o[0], o[1], o[2]));   // film_write's tone map (device_lib.h)
}

void launch_demodulate(const DenoiseParams& p, hipStream_t s) {
    hipLaunchKernelGGL(k_demodulate, denoise_grid(p), dim3(BLOCK), 0, s, p);
}
void launch_atrous(const DenoiseParams& p, const AtrousStep& a, bool ping_to_pong, hipStream_t s) {
    const float* src = ping_to_pong ? p.ping : p.pong;
    float* dst = ping_to_pong ? p.pong : p.ping;
    // steps 1 and 2 from LDS: 0.662 against 0.802 ms per 5-iteration denoise at 1920 x 1080 with the plain-load kernel throughout (MI355X,
    // two runs of two passes of 30 each way, spread 0.001 ms); from step 4 on the halo outgrows the tile and the taps read memory
    if (a.step <= 2) hipLaunchKernelGGL(k_atrous_lds, denoise_grid(p), dim3(BLOCK), 0, s, p, a, src, dst);
    else hipLaunchKernelGGL(k_atrous, denoise_grid(p), dim3(BLOCK), 0, s, p, a, src, dst);
}
void launch_demodulate_var(const DenoiseParams& p, const float* m2n, hipStream_t s) {
    hipLaunchKernelGGL(k_demodulate_var, denoise_grid(p), dim3(BLOCK), 0, s, p, m2n);
}
void launch_demodulate_resolved(const DenoiseParams& p, const float* resolved_var, hipStream_t s) {
    hipLaunchKernelGGL(k_demodulate_resolved, denoise_grid(p), dim3(BLOCK), 0, s, p, resolved_var);
}
void launch_atrous_var(const DenoiseParams& p, const AtrousVarStep& a, bool ping_to_pong, hipStream_t s) {
    const float* src = ping_to_pong ? p.ping : p.pong;
    float* dst = ping_to_pong ? p.pong : p.ping;
    // steps 1 and 2 from LDS, as launch_atrous; the tile holds a halo of 4 pixels and no more
    if (a.step <= 2) hipLaunchKernelGGL(k_atrous_var_lds, denoise_grid(p), dim3(BLOCK), 0, s, p, a, src, dst);
    else hipLaunchKernelGGL(k_atrous_var, denoise_grid(p), dim3(BLOCK), 0, s, p, a, src, dst);
}
void launch_remodulate(const DenoiseParams& p, bool from_pong, hipStream_t s) {
    hipLaunchKernelGGL(k_remodulate, denoise_grid(p), dim3(BLOCK), 0, s, p, from_pong ? p.pong : p.ping);
}

}  // namespace spc
