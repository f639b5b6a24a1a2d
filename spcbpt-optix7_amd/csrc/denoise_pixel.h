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

#include "moments_pixel.h"   // film_moments_sd: the variance-guided form starts from the film's moments

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

// ---- the variance-guided form (spcbpt_denoise_variance): a scalar variance v of the demodulated luminance rides beside c ----------
// what one iteration needs besides the planes: sigma_v^2, 1 / sigma_n^2, 1 / (sigma_x s)^2
struct AtrousVarStep {
    int step;   // s = 2^i
    float sigma_v2, inv_sigma_n2, inv_sigma_x2;
};
SPC_DN_HD AtrousVarStep atrous_var_step(int i, float sigma_v, float sigma_n, float sigma_x) {
    AtrousVarStep a;
    a.step = 1 << i;
    a.sigma_v2 = sigma_v * sigma_v;
    a.inv_sigma_n2 = 1.0f / (sigma_n * sigma_n);
    const float sx = sigma_x * (float)a.step;
    a.inv_sigma_x2 = 1.0f / (sx * sx);
    return a;
}
// v_0(p) from the film's moments m2n = (M2_r, M2_g, M2_b, n) and c0 = denoise_demodulate(accum, albedo):
//   n >= 2:  (sum_k w_k sd_k / max(albedo_k, 1e-3))^2,  sd_k = sqrt(M2_k / (n (n - 1))),  w = (0.3, 0.6, 0.1)   (moments_pixel.h)
//   n <  2:  L(c0)^2 -- a pixel whose variance is unknown counts as uncertain as its own value.  The one branch, on the integer n.
SPC_DN_HD float denoise_variance_start(const float* c0, const float* albedo, const float* m2n) {
    float s = denoise_luminance(c0);
    if (m2n[3] >= 2.0f) {
        float sd[3];
        film_moments_sd(m2n, sd);
        for (int k = 0; k < 3; k++) sd[k] = sd[k] / fmaxf(albedo[k], kDenoiseAlbedoFloor);
        s = denoise_luminance(sd);
    }
    return s * s;
}
// v_0(p) of the resolved image (spcbpt_history_denoise) from its per-channel variance RV (reproject_pixel.h: resolve_var_pixel):
//   (sum_k w_k sqrtf(RV_k) / max(albedo_k, 1e-3))^2
// the n >= 2 line above with sqrtf(RV_k) for sd_k, in its order -- where RV is the film's own variance of a pixel with n >= 2,
// sqrtf(RV_k) is sd_k and the value is denoise_variance_start's bit for bit.  No branch.
SPC_DN_HD float denoise_resolved_start(const float* albedo, const float* rv) {
    float sd[3];
    for (int k = 0; k < 3; k++) sd[k] = sqrtf(rv[k]);
    for (int k = 0; k < 3; k++) sd[k] = sd[k] / fmaxf(albedo[k], kDenoiseAlbedoFloor);
    const float s = denoise_luminance(sd);
    return s * s;
}

// One pixel of one iteration of the variance-guided filter.  `F` is atrous_pixel's, plus   float F::variance(int x, int y) const
//   v~(p)   = the (1/4, 1/2, 1/4)^2 mean of v over the 3 x 3 neighbours of p at distance 1 inside the image, renormalised
//   w(p, q) = k[a] k[b] exp(-(L(c(q)) - L(c(p)))^2 / (sigma_v^2 v~(p) + (1e-3 (1e-2 + L(c(p))))^2) - |n(q) - n(p)|^2 / sigma_n^2
//                           - |X(q) - X(p)|^2 / (sigma_x s)^2)
//   out.rgb = c(p) + sum w (c(q) - c(p)) / sum w,    out.w = sum w^2 v(q) / (sum w)^2     (the variance of that weighted mean)
// The colour term is measured in the pixel's own standard deviation, so the filter narrows as the film converges: with v = 0 only
// neighbours within a thousandth of the pixel's luminance still count.  Smooth weights only; the centre tap (w = 9 / 64) keeps the
// sum non-empty; a constant image comes back bit for bit.
template <class F>
SPC_DN_HD void atrous_var_pixel(const F& f, int x, int y, int width, int height, const AtrousVarStep& a, float* out) {
    const float kern[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    const float pre[3] = {1.0f / 4.0f, 1.0f / 2.0f, 1.0f / 4.0f};
    float cp[3], np[3], Xp[3];
    f.fetch(x, y, cp, np, Xp);
    float vs = 0.0f, gs = 0.0f;
    for (int b = -1; b <= 1; b++) {
        const int qy = y + b;
        if (qy < 0 || qy >= height) continue;
        for (int t = -1; t <= 1; t++) {
            const int qx = x + t;
            if (qx < 0 || qx >= width) continue;
            const float g = pre[t + 1] * pre[b + 1];
            vs += g * f.variance(qx, qy);
            gs += g;
        }
    }
    const float Lp = denoise_luminance(cp);
    const float floor_l = 1e-3f * (1e-2f + Lp);
    const float inv_den = 1.0f / (a.sigma_v2 * (vs / gs) + floor_l * floor_l);
    float sum[3] = {0.0f, 0.0f, 0.0f}, wsum = 0.0f, vsum = 0.0f;
    for (int b = -2; b <= 2; b++) {
        const int qy = y + a.step * b;
        if (qy < 0 || qy >= height) continue;
        for (int t = -2; t <= 2; t++) {
            const int qx = x + a.step * t;
            if (qx < 0 || qx >= width) continue;
            float cq[3], nq[3], Xq[3];
            f.fetch(qx, qy, cq, nq, Xq);
            float dc[3], dn2 = 0.0f, dx2 = 0.0f;
            for (int k = 0; k < 3; k++) {
                dc[k] = cq[k] - cp[k];
                const float dn = nq[k] - np[k], dX = Xq[k] - Xp[k];
                dn2 += dn * dn; dx2 += dX * dX;
            }
            const float dL = denoise_luminance(cq) - Lp;
            const float w = kern[t + 2] * kern[b + 2] * expf(-(dL * dL * inv_den) - dn2 * a.inv_sigma_n2 - dx2 * a.inv_sigma_x2);
            for (int k = 0; k < 3; k++) sum[k] += w * dc[k];
            wsum += w;
            vsum += w * w * f.variance(qx, qy);
        }
    }
    for (int k = 0; k < 3; k++) out[k] = cp[k] + sum[k] / wsum;
    out[3] = vsum / (wsum * wsum);
}

}  // namespace spc
