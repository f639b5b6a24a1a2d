// The per-pixel and per-node work of the local tone stage -- log-luminance, the tent weights of the bilateral grid, a node's gather, the
// grid blur, the trilinear slice, the gain -- as one set of __host__ __device__ functions shared by the kernels of
// kernels_local_tone.hip and the exported spcbpt_local_tone_host (local_tone_host.cpp, plain g++), so that all of it is testable without
// a GPU.  Float32, no contraction (the library's flags), the same operations in the same order on both sides: only + - x /, compares,
// int <-> float conversions and bit-pattern moves are on the path (no log2f / exp2f / powf / ldexpf of a maths library), so the IEEE
// device build returns the host's bits whatever the launch structure is.  Includes no device header (the bloom_pixel.h pattern).
//
// The grid is read through a functor `at(gx, gy, gz)` that returns the node's two channels: the host reads a plain array, a kernel
// reads global memory or an LDS copy of the node columns its block touches.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SPC_LT_HD __host__ __device__ inline
#else
#define SPC_LT_HD inline
#endif

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace spc {

static constexpr int kLtMaxNZ = 66;                   // floor(32 / 0.5) + 2: the bins of the finest range
static constexpr int64_t kLtMaxNodes = 1ll << 25;     // of one call's grid

struct LtNode {   // a grid node: A = sum w L, B = sum w
    float a, b;
};

SPC_LT_HD float lt_bits_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
SPC_LT_HD uint32_t lt_float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// ---- 1. log-luminance.  lt_log2(y) for a normal y > 0: e and m in [1, 2) are cut from the bit pattern, t = m - 1 (exact),
//   lt_log2 = e + P(t),   P(t) = t + t (d1 + t (c2 + t (c3 + t (c4 + t c5)))),   P(0) = 0 exactly.
// P is the least-squares degree-5 fit of log2(1 + t) on [0, 1] under P(1) = 1 (c1 = 1.4418359), written with the 1 of c1 = 1 + d1 taken
// out of the bracket: t itself then enters unrounded, and the form is non-decreasing over all 2^23 mantissas, where
// t (c1 + t (...)) steps down at 106 of them (an increment of P is 1.4 to 1.9 ulp there, the bracket's rounding is 1).
// max |lt_log2 - log2| = 1.80e-5 stops (the bar is 2^-13 = 1.22e-4).
SPC_LT_HD float lt_log2(float y) {
    const uint32_t u = lt_float_bits(y);
    const float e = (float)((int)(u >> 23) - 127);
    const float t = lt_bits_float((u & 0x007FFFFFu) | 0x3F800000u) - 1.0f;
    const float r = 0.44183588f + t * (-0.7083722f + t * (0.41355506f + t * (-0.19126251f + t * 0.04424374f)));
    return e + (t + t * r);
}

// lt_exp2(g): g clamped to [-32, 32] (a NaN goes to -32), i = floor(g), f = g - i in [0, 1],
//   lt_exp2 = Q(f) 2^i,   Q(f) = 1 + f (q1 + f (q2 + f (q3 + f q4))),   Q(0) = 1 and Q(1) = 2 exactly,
// 2^i the float whose bit pattern is (i + 127) << 23.  Q is the least-squares degree-4 fit of 2^f under Q(1) = 2; its coefficients are
// positive, so every step of the Horner form is non-decreasing in f.  max |lt_exp2 / exp2 - 1| = 4.6e-6 (the bar is 2^-13).
SPC_LT_HD float lt_exp2(float g) {
    const float c = g > -32.0f ? (g < 32.0f ? g : 32.0f) : -32.0f;
    int i = (int)c;
    if ((float)i > c) i -= 1;
    const float f = c - (float)i;
    const float q = 1.0f + f * (0.6930049f + f * (0.24153961f + f * (0.051766057f + f * 0.013689456f)));
    return q * lt_bits_float((uint32_t)(i + 127) << 23);
}

SPC_LT_HD float lt_luminance(float r, float g, float b) { return 0.3f * r + 0.6f * g + 0.1f * b; }   // display_luminance's order
SPC_LT_HD bool lt_takes_part(float Y) { return Y > 0.0f && Y < INFINITY; }                           // not NaN, zero, negative or infinite
SPC_LT_HD float lt_loglum(float Y) {                                                                 // L in [-16, 16] of a Y that takes part
    const float yc = Y < 1.52587890625e-05f ? 1.52587890625e-05f : (Y > 65536.0f ? 65536.0f : Y);
    return lt_log2(yc);
}
SPC_LT_HD float lt_bin(float L, float range) { return (L + 16.0f) / range; }   // z, the pixel's bin coordinate in [0, 32 / range]

// ---- 2. grid.  The tents: wx(d) = (float)(s - |d|) / (float)s for the offset d = x - gx s, |d| < s; wz = 1 - |z - gz| where > 0, else 0.
SPC_LT_HD float lt_tent(int d, int s) { return (float)(s - (d < 0 ? -d : d)) / (float)s; }
SPC_LT_HD float lt_tent_z(float z, int gz) {
    const float d = z - (float)gz;
    const float w = 1.0f - (d < 0.0f ? -d : d);
    return w > 0.0f ? w : 0.0f;
}
// one term of a row sum, x ascending:  a += (wx wz) L,  b += wx wz.  (A term with wz = 0 adds +-0 and changes no bit: a kernel may
// keep a pixel that takes no part as z = kLtNoBin, L = 0.)
static constexpr float kLtNoBin = -2.0f;
SPC_LT_HD void lt_row_add(LtNode& row, float wx, float z, float L, int gz) {
    const float w = wx * lt_tent_z(z, gz);
    row.a = row.a + w * L;
    row.b = row.b + w;
}
// one term of a node's sum over its rows, rows ascending:  A += wy a_j,  B += wy b_j
SPC_LT_HD void lt_node_add(LtNode& node, float wy, const LtNode& row) {
    node.a = node.a + wy * row.a;
    node.b = node.b + wy * row.b;
}

// ---- 3. blur, one axis:  out(i) = (0.25 v(i - 1) + 0.5 v(i)) + 0.25 v(i + 1), the caller clamps the indices
SPC_LT_HD float lt_blur3(float lo, float mid, float hi) { return (0.25f * lo + 0.5f * mid) + 0.25f * hi; }
SPC_LT_HD LtNode lt_blur_node(const LtNode& lo, const LtNode& mid, const LtNode& hi) { return LtNode{lt_blur3(lo.a, mid.a, hi.a), lt_blur3(lo.b, mid.b, hi.b)}; }

// ---- 4. slice: the base layer under pixel (x, y) with log-luminance L and bin coordinate z.  A and B separately: along z in each of
// the four columns, then along x in the rows iy and iy + 1, then along y.  base = A / B if B > 0, else L.
SPC_LT_HD float lt_lerp(float a, float b, float t) { return a + t * (b - a); }
SPC_LT_HD LtNode lt_lerp_node(const LtNode& p, const LtNode& q, float t) { return LtNode{lt_lerp(p.a, q.a, t), lt_lerp(p.b, q.b, t)}; }

template <class At>
SPC_LT_HD float lt_base(const At& at, int x, int y, float L, float z, int s, int nz) {
    const int ix = x / s, iy = y / s;
    const float tx = (float)(x - ix * s) / (float)s, ty = (float)(y - iy * s) / (float)s;
    int iz = (int)z;
    if (iz > nz - 2) iz = nz - 2;
    const float tz = z - (float)iz;
    const LtNode c00 = lt_lerp_node(at(ix, iy, iz), at(ix, iy, iz + 1), tz), c10 = lt_lerp_node(at(ix + 1, iy, iz), at(ix + 1, iy, iz + 1), tz);
    const LtNode c01 = lt_lerp_node(at(ix, iy + 1, iz), at(ix, iy + 1, iz + 1), tz), c11 = lt_lerp_node(at(ix + 1, iy + 1, iz), at(ix + 1, iy + 1, iz + 1), tz);
    const LtNode r0 = lt_lerp_node(c00, c10, tx), r1 = lt_lerp_node(c01, c11, tx);
    const LtNode n = lt_lerp_node(r0, r1, ty);
    return n.b > 0.0f ? n.a / n.b : L;
}

// ---- 5. gain:  g = (c - 1)(base - La) + (d - 1)(L - base);  O_rgb = I_rgb lt_exp2(g)
SPC_LT_HD float lt_gain_log(float compress, float detail, float base, float L, float La) { return (compress - 1.0f) * (base - La) + (detail - 1.0f) * (L - base); }

// the whole of steps 4 and 5 for one pixel: px[0..3] -> out[0..3].  A pixel that takes no part keeps its four floats.
template <class At>
SPC_LT_HD void lt_pixel(const At& at, int x, int y, const float* px, int s, int nz, float range, float compress, float detail, float La, float* out) {
    const float Y = lt_luminance(px[0], px[1], px[2]);
    if (!lt_takes_part(Y)) {
        out[0] = px[0]; out[1] = px[1]; out[2] = px[2]; out[3] = px[3];
        return;
    }
    const float L = lt_loglum(Y);
    const float base = lt_base(at, x, y, L, lt_bin(L, range), s, nz);
    const float k = lt_exp2(lt_gain_log(compress, detail, base, L, La));
    out[0] = px[0] * k; out[1] = px[1] * k; out[2] = px[2] * k; out[3] = px[3];
}

// ---- the grid of one call (host only: filled by local_tone_plan_of, local_tone_host.cpp, for the context and for
// spcbpt_local_tone_host alike).  Node (gx, gy, gz) is element (gy GX + gx) NZ + gz of a grid buffer, two floats (A, B) each.
struct LtPlan {
    int cell;            // s
    int gx, gy, nz;      // GX = (W - 1) / s + 2,  GY = (H - 1) / s + 2,  NZ = (int)(32 / range) + 2 (the quotient in float32)
    int64_t nodes;       // GX GY NZ
    float la;            // log2(anchor), taken in double and rounded to float once
};
LtPlan local_tone_plan_of(int width, int height, int cell, float range, float anchor);
// NULL, or what is wrong with the fields of a spcbpt_local_tone_params
const char* local_tone_params_error(int cell, float range, int blur, float compress, float detail, float anchor);

}  // namespace spc
