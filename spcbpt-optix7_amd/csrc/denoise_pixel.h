// The per-pixel work of the edge-avoiding a-trous denoiser (Dammertz et al. 2010) on the demodulated film: one set of
// __host__ __device__ functions shared by k_demodulate / k_atrous / k_remodulate (kernels_denoise.hip) and the exported
// spcbpt_denoise_host (denoise_host.cpp, plain g++), so that the filter is testable without a GPU.  Float32 throughout, no
// contraction (the library's flags), the same operations on both sides.  Includes no device header (the camera_splat.h pattern).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SPC_DN_HD __host__ __device__ inline
#else
#define SPC_DN_HD inline
#endif

#include <math.h>

namespace spc {

static constexpr float kDenoiseAlbedoFloor = 1e-3f;   // radiance / max(albedo, floor): a black texel divides by this
static constexpr int kDenoiseMaxIterations = 8;

// what one iteration needs besides the planes: 1 / (sigma_c 2^-i), 1 / sigma_n^2, 1 / (sigma_x s)^2
struct AtrousStep {
    int step;   // s = 2^i
    float inv_sigma_c, inv_sigma_n2, inv_sigma_x2;
};
SPC_DN_HD AtrousStep atrous_step(int i, float sigma_c, float sigma_n, float sigma_x) {
    AtrousStep a;
    a.step = 1 << i;
    a.inv_sigma_c = (float)a.step / sigma_c;
    a.inv_sigma_n2 = 1.0f / (sigma_n * sigma_n);
    const float sx = sigma_x * (float)a.step;
    a.inv_sigma_x2 = 1.0f / (sx * sx);
    return a;
}

// c0 = accum.rgb / max(albedo.rgb, 1e-3) per channel, and back
SPC_DN_HD void denoise_demodulate(const float* accum, const float* albedo, float* c) {
    for (int k = 0; k < 3; k++) c[k] = accum[k] / fmaxf(albedo[k], kDenoiseAlbedoFloor);
}
SPC_DN_HD void denoise_remodulate(const float* c, const float* albedo, float* out) {
    for (int k = 0; k < 3; k++) out[k] = c[k] * fmaxf(albedo[k], kDenoiseAlbedoFloor);
}
// X = d_c depth: the first hit as a point relative to the eye, d_c = camera_ray's direction with jitter 0.5 (device_lib.h)
SPC_DN_HD void denoise_position(const float* U, const float* V, const float* W, int width, int height, int x, int y, float depth, float* X) {
    const float dx = 2.0f * (((float)x + 0.5f) / (float)width) - 1.0f;
    const float dy = 2.0f * (((float)y + 0.5f) / (float)height) - 1.0f;
    const float d[3] = {dx * U[0] + dy * V[0] + W[0], dx * U[1] + dy * V[1] + W[1], dx * U[2] + dy * V[2] + W[2]};
    const float inv = 1.0f / sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    for (int k = 0; k < 3; k++) X[k] = d[k] * inv * depth;
}
SPC_DN_HD float denoise_luminance(const float* c) { return 0.3f * c[0] + 0.6f * c[1] + 0.1f * c[2]; }

// One pixel of one iteration.  `F` hands out the three guides of a pixel INSIDE the image, from wherever the caller keeps them
// (global planes, an LDS tile, host arrays):   void F::fetch(int x, int y, float c[3], float n[3], float X[3]) const
//   w(p, q) = k[a] k[b] exp(-|c(q) - c(p)|^2 / ((sigma_c 2^-i)^2 (1e-2 + (L(c(p)) + L(c(q))) / 2)^2) - |n(q) - n(p)|^2 / sigma_n^2
//                           - |X(q) - X(p)|^2 / (sigma_x s)^2),        q = p + s (a, b),  a, b in -2 .. 2,  k = (1, 4, 6, 4, 1) / 16
//   out = sum w c(q) / sum w      (taps outside the image are skipped; the centre tap has w = 9 / 64, so the sum is never empty)
// evaluated as c(p) + sum w (c(q) - c(p)) / sum w: the same value, and a constant image comes back bit for bit.
// Smooth weights only -- no threshold, no division by a guide -- so a float64 recomputation never disagrees on a decision.
template <class F>
SPC_DN_HD void atrous_pixel(const F& f, int x, int y, int width, int height, const AtrousStep& a, float* out) {
    const float kern[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float cp[3], np[3], Xp[3];
    f.fetch(x, y, cp, np, Xp);
    const float Lp = denoise_luminance(cp);
    float sum[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f;
    for (int b = -2; b <= 2; b++) {
        const int qy = y + a.step * b;
        if (qy < 0 || qy >= height) continue;
        for (int t = -2; t <= 2; t++) {
            const int qx = x + a.step * t;
            if (qx < 0 || qx >= width) continue;
            float cq[3], nq[3], Xq[3];
            f.fetch(qx, qy, cq, nq, Xq);
            float dc[3], dc2 = 0.0f, dn2 = 0.0f, dx2 = 0.0f;
            for (int k = 0; k < 3; k++) {
                dc[k] = cq[k] - cp[k];
                const float dn = nq[k] - np[k], dX = Xq[k] - Xp[k];
                dc2 += dc[k] * dc[k]; dn2 += dn * dn; dx2 += dX * dX;
            }
            const float lum = 1e-2f + 0.5f * (Lp + denoise_luminance(cq));
            const float rc = a.inv_sigma_c / lum;
            const float w = kern[t + 2] * kern[b + 2] * expf(-(dc2 * (rc * rc)) - dn2 * a.inv_sigma_n2 - dx2 * a.inv_sigma_x2);
            for (int k = 0; k < 3; k++) sum[k] += w * dc[k];
            wsum += w;
        }
    }
    for (int k = 0; k < 3; k++) out[k] = cp[k] + sum[k] / wsum;
}

}  // namespace spc
