// The thin-lens camera (spcbpt_set_lens): a finite aperture of radius `radius` (world units) in the plane through `eye` spanned by U and
// V, focused on the plane g = focus (depth along W in units of W: camera_splat.h).  Two forms of ONE camera, written apart on purpose:
//   camera_lens_ray    the START of an eye sub-path ("SPCBPT_eye", "pt"): pixel sample + lens sample -> origin, direction
//   camera_splat_lens  the END of a light sub-path ("lt", BDPT strategy t = 1): world point + lens sample -> pixel, importance
// __host__ __device__, shared by the kernels (dev_lens.h, dev_splat.h) and the exported host forms (ctx_lens.hip), so that both are
// testable without a GPU.  Float32 throughout, no contraction (the library's flags), the same operations on both sides -- the two
// trigonometric values of the disc map included (lens_sin_q / lens_cos_q below: no libm, no device library).
// radius == 0 is the pinhole: camera_ray's direction from `eye` and camera_splat's answer, bit for bit; `focus` is ignored.
#pragma once
#include "camera_splat.h"

namespace spc {

// Sine and cosine on [-pi/4, pi/4], the only arguments the disc map has: the single-precision minimax kernels of Cephes (sinf.c / cosf.c,
// S. Moshier; peak relative error 2^-23 on this interval) written out as + and x, so that host and device compute the SAME bits -- and
// the device pays no argument reduction, whose registers the eye megakernel does not have.
SPC_CS_HD float lens_sin_q(float x) {
    const float z = x * x;
    return ((-1.9515295891e-4f * z + 8.3321608736e-3f) * z - 1.6666654611e-1f) * z * x + x;
}
SPC_CS_HD float lens_cos_q(float x) {
    const float z = x * x;
    return ((2.443315711809948e-5f * z - 1.388731625493765e-3f) * z + 4.166664568298827e-2f) * z * z - 0.5f * z + 1.0f;
}

// The concentric map (Shirley & Chiu 1997) of the unit square onto the unit disc: area-preserving, so uniform (u1, u2) give a uniform
// point (a, b).  With (sx, sy) = 2 (u1, u2) - 1: |sx| > |sy|: r = sx, phi = (pi/4) sy / sx; otherwise r = sy, phi = pi/2 - (pi/4) sx / sy
// -- whose cosine and sine are the sine and cosine of psi = (pi/4) sx / sy, so both arms evaluate the kernels on [-pi/4, pi/4].
// |(a, b)| = max(|sx|, |sy|) <= 1 up to the rounding of the two kernels.
SPC_CS_HD void lens_disc(float u1, float u2, float& a, float& b) {
    const float sx = 2.0f * u1 - 1.0f, sy = 2.0f * u2 - 1.0f;
    if (sx == 0.0f && sy == 0.0f) { a = 0.0f; b = 0.0f; return; }
    const bool wide = fabsf(sx) > fabsf(sy);
    const float r = wide ? sx : sy;
    const float psi = 0.78539816339744830962f * (wide ? sy / sx : sx / sy);
    const float c = lens_cos_q(psi), s = lens_sin_q(psi);
    a = r * (wide ? c : s);
    b = r * (wide ? s : c);
}

// The lens point relative to the eye: off = a Lu + b Lv with the lens axes Lu = radius U / |U|, Lv = radius V / |V|.  The axes belong to
// the camera, not to the sample: the host computes them once (Context::update_lens_axes) and hands them to the kernels, which then
// evaluate camera_lens_point alone -- the same bits as the host forms below, which compute both.
SPC_CS_HD void camera_lens_axes(const float* U, const float* V, float radius, float* Lu, float* Lv) {
    const float ul = sqrtf(U[0] * U[0] + U[1] * U[1] + U[2] * U[2]), vl = sqrtf(V[0] * V[0] + V[1] * V[1] + V[2] * V[2]);
    for (int k = 0; k < 3; k++) { Lu[k] = radius * (U[k] / ul); Lv[k] = radius * (V[k] / vl); }
}
SPC_CS_HD void camera_lens_point(const float* Lu, const float* Lv, float u1, float u2, float* off) {
    float a, b;
    lens_disc(u1, u2, a, b);
    for (int k = 0; k < 3; k++) off[k] = a * Lu[k] + b * Lv[k];
}
SPC_CS_HD void camera_lens_offset(const float* U, const float* V, float u1, float u2, float radius, float* off) {
    float Lu[3], Lv[3];
    camera_lens_axes(U, V, radius, Lu, Lv);
    camera_lens_point(Lu, Lv, u1, u2, off);
}

// Pixel (x, y), jitter (jx, jy), lens numbers (u1, u2): the ray from the lens point O = eye + off through the sample's focus point
// F = eye + focus (dx U + dy V + W), dx and dy as in camera_ray (device_lib.h).  F - O is formed as focus d - off: `eye` cancels exactly.
SPC_CS_HD void camera_lens_ray_axes(const float* eye, const float* U, const float* V, const float* W, int width, int height, int x, int y,
                                    float jx, float jy, float u1, float u2, const float* Lu, const float* Lv, float focus, float* origin, float* dir) {
    const float dx = 2.0f * (((float)x + jx) / (float)width) - 1.0f;
    const float dy = 2.0f * (((float)y + jy) / (float)height) - 1.0f;
    float d[3], off[3];
    for (int k = 0; k < 3; k++) d[k] = dx * U[k] + dy * V[k] + W[k];
    camera_lens_point(Lu, Lv, u1, u2, off);
    for (int k = 0; k < 3; k++) { origin[k] = eye[k] + off[k]; d[k] = focus * d[k] - off[k]; }
    const float inv = 1.0f / sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);   // (normalize of device_lib.h)
    for (int k = 0; k < 3; k++) dir[k] = d[k] * inv;
}
SPC_CS_HD void camera_lens_ray(const float* eye, const float* U, const float* V, const float* W, int width, int height, int x, int y,
                               float jx, float jy, float u1, float u2, float radius, float focus, float* origin, float* dir) {
    if (radius > 0.0f) {
        float Lu[3], Lv[3];
        camera_lens_axes(U, V, radius, Lu, Lv);
        camera_lens_ray_axes(eye, U, V, W, width, height, x, y, jx, jy, u1, u2, Lu, Lv, focus, origin, dir);
        return;
    }
    const float dx = 2.0f * (((float)x + jx) / (float)width) - 1.0f;   // camera_ray (device_lib.h)
    const float dy = 2.0f * (((float)y + jy) / (float)height) - 1.0f;
    float d[3];
    for (int k = 0; k < 3; k++) { d[k] = dx * U[k] + dy * V[k] + W[k]; origin[k] = eye[k]; }
    const float inv = 1.0f / sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    for (int k = 0; k < 3; k++) dir[k] = d[k] * inv;
}

// A world point seen through the lens point O = eye + off (off in the lens plane, so the depth g of a point is the same from O as from
// the eye).  With c = point - O and g = c . (U x V) / D:
//   g <= 0                         behind the lens plane: rejected
//   q  = (focus / g) c             from O to F, the point where the line O -> point meets the plane g = focus
//   (dx, dy) = those of F          camera_project of off + q = F - eye; outside the image: rejected
//   weight = w h |q|^3 / (4 focus^2 |q . (U x V)|), q . (U x V) = focus D
//                                  the reciprocal solid angle, seen from O, of the pixel's footprint on the focus plane: a parallelogram
//                                  of area (2 / w)(2 / h) focus^2 |U x V|, |q| away and tilted by |q . (U x V)| / (|U x V| |q|)
// With off = 0 and focus = 1 that is camera_splat's w h |c / g|^3 / (4 |D|).
SPC_CS_HD bool camera_splat_lens_at(const float* eye, const float* U, const float* V, const float* W, int width, int height, const float* point,
                                    const float* off, float focus, float& dx, float& dy, int& px, int& py, float& weight) {
    const float O[3] = {eye[0] + off[0], eye[1] + off[1], eye[2] + off[2]};
    const CameraProjection pc = camera_project(O, U, V, W, point);
    if (!(pc.g > 0.0f)) return false;
    const float s = focus / pc.g;
    const float q[3] = {s * pc.c[0], s * pc.c[1], s * pc.c[2]};
    const float f[3] = {off[0] + q[0], off[1] + q[1], off[2] + q[2]};   // F - eye
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    const CameraProjection pf = camera_project(zero, U, V, W, f);
    const float x = pf.dx, y = pf.dy;
    if (!(fabsf(x) < 1.0f && fabsf(y) < 1.0f)) return false;
    int ix = (int)floorf((x + 1.0f) * 0.5f * (float)width), iy = (int)floorf((y + 1.0f) * 0.5f * (float)height);
    ix = ix < 0 ? 0 : (ix > width - 1 ? width - 1 : ix);
    iy = iy < 0 ? 0 : (iy > height - 1 ? height - 1 : iy);
    const float r = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    const float we = (float)width * (float)height * (r * r * r) / (4.0f * (focus * focus) * fabsf(focus * pc.D));
    dx = x; dy = y; px = ix; py = iy; weight = we;
    return true;
}

// Returns false (and writes nothing) when the point does not land inside the image.
SPC_CS_HD bool camera_splat_lens(const float* eye, const float* U, const float* V, const float* W, int width, int height, const float* point,
                                 float u1, float u2, float radius, float focus, float& dx, float& dy, int& px, int& py, float& weight) {
    if (!(radius > 0.0f)) return camera_splat(eye, U, V, W, width, height, point, dx, dy, px, py, weight);
    float off[3];
    camera_lens_offset(U, V, u1, u2, radius, off);
    return camera_splat_lens_at(eye, U, V, W, width, height, point, off, focus, dx, dy, px, py, weight);
}

}  // namespace spc
