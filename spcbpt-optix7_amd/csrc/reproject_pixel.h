// The per-pixel work of the depth-based history reprojection (include/spcbpt.h: spcbpt_history_*): one set of __host__ __device__
// functions shared by k_reproject / k_resolve (kernels_reproject.hip) and the exported spcbpt_history_reproject_host /
// spcbpt_history_resolve_host (reproject_host.cpp, plain g++), so that the pass is testable without a GPU.  Float32 throughout, no
// contraction (the library's flags), the same operations on both sides.  Includes no device header (the camera_splat.h pattern).
#pragma once
#include <math.h>

#include "camera_splat.h"    // camera_project: where a world point lands in the history camera
#include "denoise_pixel.h"   // denoise_position: the first hit of a pixel's centre ray, relative to the eye

namespace spc {

struct ReprojectCamera {   // spcbpt_set_camera's four vectors
    float eye[3], U[3], V[3], W[3];
};
struct ReprojectStep {     // the parameters with their defaults resolved: 1 / sigma_n^2, 1 / sigma_x^2, max_history
    float inv_sigma_n2, inv_sigma_x2, max_history;
};
SPC_DN_HD ReprojectStep reproject_step(float sigma_n, float sigma_x, float max_history) {
    ReprojectStep s;
    s.inv_sigma_n2 = 1.0f / (sigma_n * sigma_n);
    s.inv_sigma_x2 = 1.0f / (sigma_x * sigma_x);
    s.max_history = max_history;
    return s;
}

// where the history is sampled for a point that landed at (dx, dy): f = clamp((d + 1) / 2 size - 0.5, -2, size + 1), its floor and
// its fraction.  The clamp keeps the integer conversion defined; a clamped coordinate has both taps outside the image.
SPC_DN_HD void reproject_tap(float d, int size, int& i0, float& a) {
    const float f = fminf(fmaxf((d + 1.0f) * 0.5f * (float)size - 0.5f, -2.0f), (float)size + 1.0f);
    const float fl = floorf(f);
    i0 = (int)fl;
    a = f - fl;
}

// One pixel of the prior.  `F` hands out the two history planes of a pixel INSIDE the image, from wherever the caller keeps them
// (global planes, host arrays):   void F::fetch(int x, int y, float g[4], float h[4]) const     G(q) = (normal, depth), H(q) = (rgb, n)
//   nd.w <= 0 (a miss): R = 0.     P = eye + denoise_position(U, V, W, x, y, nd.w)
//   (g, dx, dy) = camera_project(history camera, P);     g <= 0: R = 0
//   the four taps q = (x0 + i, y0 + j) of reproject_tap; outside the image or G(q).w <= 0: weight 0, else
//   X_q = eye_h + denoise_position(U_h, V_h, W_h, q, G(q).w)
//   w_q = b_q exp(-(nd.xyz . (X_q - P))^2 / sigma_x^2 - |G(q).xyz - nd.xyz|^2 / sigma_n^2),    b_q the bilinear weight
//   S = sum w_q,  C = sum w_q H(q).rgb,  N = sum w_q H(q).n;     S < 1e-6: R = 0, else R = (C / S, S min(N / S, max_history))
// Smooth weights only: the decisions on computed values are g <= 0 (every tap is outside then) and the S cut (a jump of 1e-6 frames).
template <class F>
SPC_DN_HD void reproject_pixel(const F& f, const ReprojectCamera& cur, const ReprojectCamera& hist, int width, int height, int x, int y,
                               const float* nd, const ReprojectStep& s, float* out) {
    out[0] = out[1] = out[2] = out[3] = 0.0f;
    if (!(nd[3] > 0.0f)) return;
    float P[3];
    denoise_position(cur.U, cur.V, cur.W, width, height, x, y, nd[3], P);
    for (int k = 0; k < 3; k++) P[k] = cur.eye[k] + P[k];
    const CameraProjection pr = camera_project(hist.eye, hist.U, hist.V, hist.W, P);
    if (!(pr.g > 0.0f)) return;
    int x0, y0;
    float ax, ay;
    reproject_tap(pr.dx, width, x0, ax);
    reproject_tap(pr.dy, height, y0, ay);
    float S = 0.0f, C[3] = {0.0f, 0.0f, 0.0f}, N = 0.0f;
    for (int j = 0; j < 2; j++) {
        const int qy = y0 + j;
        if (qy < 0 || qy >= height) continue;
        for (int i = 0; i < 2; i++) {
            const int qx = x0 + i;
            if (qx < 0 || qx >= width) continue;
            float G[4], H[4];
            f.fetch(qx, qy, G, H);
            if (!(G[3] > 0.0f)) continue;
            const float b = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
            float X[3];
            denoise_position(hist.U, hist.V, hist.W, width, height, qx, qy, G[3], X);
            float plane = 0.0f, dn2 = 0.0f;
            for (int k = 0; k < 3; k++) {
                const float dX = (hist.eye[k] + X[k]) - P[k], dn = G[k] - nd[k];
                plane += nd[k] * dX;
                dn2 += dn * dn;
            }
            const float w = b * expf(-(plane * plane) * s.inv_sigma_x2 - dn2 * s.inv_sigma_n2);
            S += w;
            for (int k = 0; k < 3; k++) C[k] += w * H[k];
            N += w * H[3];
        }
    }
    if (S < 1e-6f) return;
    for (int k = 0; k < 3; k++) out[k] = C[k] / S;
    out[3] = S * fminf(N / S, s.max_history);
}

// One pixel of the resolve: the prior (worth m = prior.w frames) blended with the film's mean of `frames` frames
//   out.rgb = (m prior.rgb + Nf accum.rgb) / (m + Nf),   out.w = m + Nf,   Nf = (float)frames >= 1
// Without a prior (NULL: m = 0 everywhere) that is accum.rgb, and it is handed out as such: the film bit for bit, whatever Nf.
SPC_DN_HD void resolve_pixel(const float* prior, const float* accum, float nf, float* out) {
    if (!prior) {
        for (int k = 0; k < 3; k++) out[k] = accum[k];
        out[3] = nf;
        return;
    }
    const float m = prior[3], den = m + nf;
    for (int k = 0; k < 3; k++) out[k] = (m * prior[k] + nf * accum[k]) / den;
    out[3] = den;
}

// ---- the variance of what is shown (spcbpt_history_denoise): per channel, the variance of the MEAN of a pixel -----------------------
// VA(p), the film's own, from accum and the moments plane m2n = (M2, n):
//   n >= 2:  VA_k = max(M2_k, 0) / (n (n - 1))     film_moments_sd's operations in its order, so that sqrtf(VA_k) is sd_k bit for bit
//   n <  2:  VA_k = accum_k^2                      unknown: as uncertain as its own value (denoise_variance_start's rule, per channel)
// The one branch, on the integer n.
SPC_DN_HD void film_variance(const float* accum, const float* m2n, float* va) {
    if (m2n[3] >= 2.0f) {
        const float nn = m2n[3] * (m2n[3] - 1.0f);
        for (int k = 0; k < 3; k++) va[k] = fmaxf(m2n[k], 0.0f) / nn;
    } else {
        for (int k = 0; k < 3; k++) va[k] = accum[k] * accum[k];
    }
}

// One pixel of the prior AND of its variance: reproject_pixel's taps, weights and sums, computed once, with a second payload.  `F` is
// reproject_pixel's, with a third plane:   void F::fetch(int x, int y, float g[4], float h[4], float hv[4]) const     HV(q) = variance of H(q).rgb
//   out = reproject_pixel's R(p), operation for operation (the same bits);     PV_k = sum_q w_q HV_k(q) / S,   0 wherever R(p) = 0
// The interpolation is LINEAR in the variance, not w_q^2: neighbouring history pixels share light sub-paths and the taps of earlier
// interpolations, so they are not independent samples, and the w^2 rule would understate the variance of their mean by up to 4 x.
// max_history clamps what the prior is worth (m), not how uncertain its value is: PV is not rescaled by it.
template <class F>
SPC_DN_HD void reproject_var_pixel(const F& f, const ReprojectCamera& cur, const ReprojectCamera& hist, int width, int height, int x, int y,
                                   const float* nd, const ReprojectStep& s, float* out, float* out_var) {
    out[0] = out[1] = out[2] = out[3] = 0.0f;
    out_var[0] = out_var[1] = out_var[2] = out_var[3] = 0.0f;
    if (!(nd[3] > 0.0f)) return;
    float P[3];
    denoise_position(cur.U, cur.V, cur.W, width, height, x, y, nd[3], P);
    for (int k = 0; k < 3; k++) P[k] = cur.eye[k] + P[k];
    const CameraProjection pr = camera_project(hist.eye, hist.U, hist.V, hist.W, P);
    if (!(pr.g > 0.0f)) return;
    int x0, y0;
    float ax, ay;
    reproject_tap(pr.dx, width, x0, ax);
    reproject_tap(pr.dy, height, y0, ay);
    float S = 0.0f, C[3] = {0.0f, 0.0f, 0.0f}, N = 0.0f, D[3] = {0.0f, 0.0f, 0.0f};
    for (int j = 0; j < 2; j++) {
        const int qy = y0 + j;
        if (qy < 0 || qy >= height) continue;
        for (int i = 0; i < 2; i++) {
            const int qx = x0 + i;
            if (qx < 0 || qx >= width) continue;
            float G[4], H[4], HV[4];
            f.fetch(qx, qy, G, H, HV);
            if (!(G[3] > 0.0f)) continue;
            const float b = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
            float X[3];
            denoise_position(hist.U, hist.V, hist.W, width, height, qx, qy, G[3], X);
            float plane = 0.0f, dn2 = 0.0f;
            for (int k = 0; k < 3; k++) {
                const float dX = (hist.eye[k] + X[k]) - P[k], dn = G[k] - nd[k];
                plane += nd[k] * dX;
                dn2 += dn * dn;
            }
            const float w = b * expf(-(plane * plane) * s.inv_sigma_x2 - dn2 * s.inv_sigma_n2);
            S += w;
            for (int k = 0; k < 3; k++) C[k] += w * H[k];
            N += w * H[3];
            for (int k = 0; k < 3; k++) D[k] += w * HV[k];
        }
    }
    if (S < 1e-6f) return;
    for (int k = 0; k < 3; k++) out[k] = C[k] / S;
    out[3] = S * fminf(N / S, s.max_history);
    for (int k = 0; k < 3; k++) out_var[k] = D[k] / S;
}

// One pixel of the resolve with its variance: out is resolve_pixel's (the same bits), and with m = prior.w, Nf as there
//   RV_k = (m^2 PV_k + Nf^2 VA_k) / (m + Nf)^2      the variance of the blend of two independent means
// VA = film_variance(accum, m2n): the moments plane's own n says how well the film is known, `frames` only weights, as in the blend.
// Without a prior (NULL, both) RV is VA, handed out as such -- bit for bit, not the formula with m = 0.
SPC_DN_HD void resolve_var_pixel(const float* prior, const float* prior_var, const float* accum, const float* m2n, float nf, float* out, float* out_var) {
    resolve_pixel(prior, accum, nf, out);
    float va[3];
    film_variance(accum, m2n, va);
    out_var[3] = 0.0f;
    if (!prior) {
        for (int k = 0; k < 3; k++) out_var[k] = va[k];
        return;
    }
    const float m = prior[3], den = m + nf;
    const float m2 = m * m, nf2 = nf * nf, den2 = den * den;
    for (int k = 0; k < 3; k++) out_var[k] = (m2 * prior_var[k] + nf2 * va[k]) / den2;
}

}  // namespace spc
