// The per-texel work of the bloom stage -- what may be redistributed, the 4x4 down filter, the bilinear up filter with the level mix,
// the composite -- as one set of __host__ __device__ functions shared by the kernels of kernels_bloom.hip and the exported
// spcbpt_bloom_host (bloom_host.cpp, plain g++), so that all of it is testable without a GPU.  Float32, no contraction (the library's
// flags), the same operations in the same order on both sides: only + - x /, min and compare are on the path, so the IEEE device build
// returns the host's bits whatever the launch structure is.  Includes no device header (the display_pixel.h pattern).
//
// A level is read through a functor `at(x, y)` that takes UNCLAMPED texel coordinates and returns the texel at the coordinates clamped
// to the level's edge: the host reads a plain array, a kernel reads global memory or an LDS tile that was filled with clamped texels.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SPC_BP_HD __host__ __device__ inline
#else
#define SPC_BP_HD inline
#endif

#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace spc {

static constexpr int kBloomMaxLevels = 8;

struct BloomPx {
    float r, g, b;
};

SPC_BP_HD int bloom_clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }   // to [0, hi]

// ---- 1. what may be redistributed:  C = I > 0 ? min(I, K) : 0 (NaN and negatives give 0, +inf gives K),  Y = 0.3 Cr + 0.6 Cg + 0.1 Cb,
// t = Y > T ? (Y - T) / Y : 0,  P = C t.  With T = 0, t is exactly 1 wherever Y > 0 and P = C.
SPC_BP_HD float bloom_clip(float c, float K) { return c > 0.0f ? (c < K ? c : K) : 0.0f; }

SPC_BP_HD BloomPx bloom_pre(float r, float g, float b, float T, float K) {
    const float cr = bloom_clip(r, K), cg = bloom_clip(g, K), cb = bloom_clip(b, K);
    const float Y = 0.3f * cr + 0.6f * cg + 0.1f * cb;   // the project's weights, in display_luminance's order
    const float t = Y > T ? (Y - T) / Y : 0.0f;
    return BloomPx{cr * t, cg * t, cb * t};
}

// ---- 2. down: D_{k+1}(x, y) = sum_j sum_i w_j w_i D_k(cx(2x - 1 + i), cy(2y - 1 + j)), w = (1, 3, 3, 1) / 8.  The four horizontal sums
// first, each ((w0 a0 + w1 a1) + w2 a2) + w3 a3, then the same form down the column.
SPC_BP_HD float bloom_sum4(float a0, float a1, float a2, float a3) { return ((0.125f * a0 + 0.375f * a1) + 0.375f * a2) + 0.125f * a3; }

template <class At>
SPC_BP_HD BloomPx bloom_down_row(const At& at, int x, int sy) {   // one horizontal sum: output column x, source row sy (unclamped)
    const BloomPx a0 = at(2 * x - 1, sy), a1 = at(2 * x, sy), a2 = at(2 * x + 1, sy), a3 = at(2 * x + 2, sy);
    return BloomPx{bloom_sum4(a0.r, a1.r, a2.r, a3.r), bloom_sum4(a0.g, a1.g, a2.g, a3.g), bloom_sum4(a0.b, a1.b, a2.b, a3.b)};
}

SPC_BP_HD BloomPx bloom_down_col(const BloomPx& h0, const BloomPx& h1, const BloomPx& h2, const BloomPx& h3) {
    return BloomPx{bloom_sum4(h0.r, h1.r, h2.r, h3.r), bloom_sum4(h0.g, h1.g, h2.g, h3.g), bloom_sum4(h0.b, h1.b, h2.b, h3.b)};
}

template <class At>
SPC_BP_HD BloomPx bloom_down(const At& at, int x, int y) {
    const BloomPx h0 = bloom_down_row(at, x, 2 * y - 1), h1 = bloom_down_row(at, x, 2 * y), h2 = bloom_down_row(at, x, 2 * y + 1),
                  h3 = bloom_down_row(at, x, 2 * y + 2);
    return bloom_down_col(h0, h1, h2, h3);
}

SPC_BP_HD BloomPx bloom_scale(float g, const BloomPx& a) { return BloomPx{g * a.r, g * a.g, g * a.b}; }   // U_L = g_L D_L

// ---- 3. up: up(A)(x, y) at the size of the finer level: px = x >> 1, nx = clamp(px + (x & 1 ? 1 : -1)); horizontally
// 0.75 A(px) + 0.25 A(nx) on the rows py and ny, then the same vertically over those two.
SPC_BP_HD float bloom_lerp(float near_, float far_) { return 0.75f * near_ + 0.25f * far_; }

template <class At>
SPC_BP_HD BloomPx bloom_up(const At& at, int x, int y) {
    const int px = x >> 1, nx = px + ((x & 1) ? 1 : -1), py = y >> 1, ny = py + ((y & 1) ? 1 : -1);
    const BloomPx a = at(px, py), b = at(nx, py), c = at(px, ny), d = at(nx, ny);
    const float h0r = bloom_lerp(a.r, b.r), h0g = bloom_lerp(a.g, b.g), h0b = bloom_lerp(a.b, b.b);
    const float h1r = bloom_lerp(c.r, d.r), h1g = bloom_lerp(c.g, d.g), h1b = bloom_lerp(c.b, d.b);
    return BloomPx{bloom_lerp(h0r, h1r), bloom_lerp(h0g, h1g), bloom_lerp(h0b, h1b)};
}

// U_k = g_k D_k + up(U_{k+1})
SPC_BP_HD BloomPx bloom_mix(float g, const BloomPx& d, const BloomPx& up) { return BloomPx{g * d.r + up.r, g * d.g + up.g, g * d.b + up.b}; }

// ---- 4. composite: O = I + s (B - P), per channel; alpha is the source's.  A NaN stays in its channel (its P is 0), +inf stays +inf.
SPC_BP_HD float bloom_composite(float i, float s, float b, float p) { return i + s * (b - p); }

// ---- the pyramid of one call (host only: filled by bloom_plan_of, bloom_host.cpp, for the context and for spcbpt_bloom_host alike).
// Level 0 is the source; level k = 1 .. levels is ceil(w_{k-1} / 2) x ceil(h_{k-1} / 2) and starts `off[k]` texels into the scratch.
// g[k]: the level weights q^(k-1) / sum_m q^(m-1), computed in double and rounded to float once.
struct BloomPlan {
    int levels;
    int w[kBloomMaxLevels + 1], h[kBloomMaxLevels + 1];
    size_t off[kBloomMaxLevels + 1];
    size_t texels;                       // of the levels 1 .. levels together
    float g[kBloomMaxLevels + 1];
};
BloomPlan bloom_plan_of(int width, int height, int levels, float spread);
// NULL, or what is wrong with the fields of a spcbpt_bloom_params
const char* bloom_params_error(int levels, float strength, float spread, float threshold, float clamp);

}  // namespace spc
