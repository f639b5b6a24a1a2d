// The per-bounce arithmetic of the reflected denoiser guides: one set of __host__ __device__ functions shared by k_guides
// (kernels_guides.hip, through dev_guides.h) and the exported spcbpt_guide_step_host (guides_host.cpp, plain g++), so that the rule
// that decides which hits are followed, the reflected direction, the mirror's tint and the unfolding of what is seen behind it are
// testable without a GPU.  Float32 throughout, no contraction (the library's flags); + - * / and compares only, so that host and device
// agree bit for bit.  Includes no device header (the denoise_pixel.h pattern).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SPC_GS_HD __host__ __device__ inline
#else
#define SPC_GS_HD inline
#endif

#include <stdint.h>

namespace spc {

// A surface hit is followed iff it is mirror-like: both compares are false for a NaN, so a NaN material is never followed.
SPC_GS_HD bool guide_followed(float roughness, float metallic, float roughness_max, float metallic_min) {
    return roughness <= roughness_max && metallic >= metallic_min;
}

// v - 2 (v.N) N: the reflection of `v` about the plane of unit normal N.  With v the ray direction it is the next segment's direction;
// with v a normal found behind the mirror it carries that normal back through the mirror (the unfolding); with v a row of the running
// composition M = H_1 H_2 ... H_k (H_i = I - 2 N_i N_i^T) it is that row of M H_{k+1}.  `out` may be `v`.
SPC_GS_HD void guide_reflect(const float* v, const float* N, float* out) {
    const float d = v[0] * N[0] + v[1] * N[1] + v[2] * N[2];
    const float s = 2.0f * d;
    const float x = v[0] - s * N[0], y = v[1] - s * N[1], z = v[2] - s * N[2];
    out[0] = x; out[1] = y; out[2] = z;
}

// M <- M H(N), row by row; M is row-major 3 x 3.
SPC_GS_HD void guide_compose(float* M, const float* N) {
    guide_reflect(M, N, M);
    guide_reflect(M + 3, N, M + 3);
    guide_reflect(M + 6, N, M + 6);
}

// M n: a normal found behind the mirrors of M, carried back through them in reverse order (H_1 (H_2 (... (H_k n))))
SPC_GS_HD void guide_unfold(const float* M, const float* n, float* out) {
    const float x = M[0] * n[0] + M[1] * n[1] + M[2] * n[2];
    const float y = M[3] * n[0] + M[4] * n[1] + M[5] * n[2];
    const float z = M[6] * n[0] + M[7] * n[1] + M[8] * n[2];
    out[0] = x; out[1] = y; out[2] = z;
}

// The factor a mirror puts on what it reflects: the specular Fresnel colour Fs of bsdf_eval (dev_bsdf.h) at the mirror configuration
// H = N, where L.H = |N.dir|:  lerp3(Cspec0, 1, schlick(|N.dir|)),  Cspec0 = lerp3(specular 0.08 lerp3(1, Ctint, specularTint), base,
// metallic),  Ctint = base / lum (1 for lum <= 0) -- operation for operation bsdf_eval's (operator/(f3, float) multiplies by the
// reciprocal; lerp is a + t (b - a); schlick clamps 1 - u to [0, 1] and takes the fifth power as (m^2)^2 m).
SPC_GS_HD void guide_tint(const float* base, float metallic, float specular, float specular_tint, float n_dot_dir, float* tint) {
    const float lum = 0.3f * base[0] + 0.6f * base[1] + 0.1f * base[2];
    const float inv = 1.0f / lum;
    const float u = n_dot_dir < 0.0f ? -n_dot_dir : n_dot_dir;
    float m = 1.0f - u;
    m = m < 1.0f ? m : 1.0f;      // clampf(1 - u, 0, 1) = fmaxf(0, fminf(1 - u, 1))
    m = m > 0.0f ? m : 0.0f;
    const float m2 = m * m;
    const float F = m2 * m2 * m;
    for (int k = 0; k < 3; k++) {
        const float ctint = lum > 0.0f ? base[k] * inv : 1.0f;
        const float white = 1.0f + specular_tint * (ctint - 1.0f);
        const float s0 = specular * 0.08f * white;
        const float c0 = s0 + metallic * (base[k] - s0);
        tint[k] = c0 + F * (1.0f - c0);
    }
}

}  // namespace spc
