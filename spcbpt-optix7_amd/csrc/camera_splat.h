// The camera as the END of a light sub-path (BDPT strategy t = 1): where a world point lands on the film and with what importance.
// One __host__ __device__ function, shared by k_lt_splat (dev_splat.h) and the exported spcbpt_camera_splat (ctx_splat.hip), so that
// the projection is testable without a GPU.  Float32 throughout, no contraction (the library's flags), the same operations on both sides.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SPC_CS_HD __host__ __device__ inline
#else
#define SPC_CS_HD inline   // plain g++ (reproject_host.cpp): the same functions without the HIP headers
#endif

#include <math.h>

namespace spc {

// camera_ray (device_lib.h) shoots pixel (x, y), jitter (jx, jy) along dx U + dy V + W with dx = 2 (x + jx) / w - 1, dy likewise.  The
// inverse, for any U, V, W with D = U . (V x W) != 0 (orthogonal or not), with c = point - eye:
//   g  = c . (U x V) / D                  depth along W in units of W (g <= 0: behind the camera or in the eye plane)
//   dx = (c . (V x W) / D) / g            dy = (c . (W x U) / D) / g           (|dx| >= 1 or |dy| >= 1: outside the image)
//   px = floor((dx + 1) / 2 w)            py = floor((dy + 1) / 2 h)           (row 0 at dy = -1)
//   weight = w h |c / g|^3 / (4 |D|)      the reciprocal solid angle of a pixel seen along c: the pixel's parallelogram on the plane
//                                         g = 1 has area (2 / w)(2 / h) |U x V|, lies |c / g| away and is tilted by D / (|U x V| |c / g|)
// camera_project is that algebra alone -- c, D, g, dx, dy, whatever g is (dx and dy mean nothing unless g > 0) -- shared by camera_splat
// below and by the history reprojection (reproject_pixel.h), which lands a first hit in an EARLIER camera.
struct CameraProjection {
    float c[3], D, g, dx, dy;
};
SPC_CS_HD CameraProjection camera_project(const float* eye, const float* U, const float* V, const float* W, const float* point) {
    CameraProjection r;
    r.c[0] = point[0] - eye[0]; r.c[1] = point[1] - eye[1]; r.c[2] = point[2] - eye[2];
    const float* c = r.c;
    const float vw[3] = {V[1] * W[2] - V[2] * W[1], V[2] * W[0] - V[0] * W[2], V[0] * W[1] - V[1] * W[0]};
    const float wu[3] = {W[1] * U[2] - W[2] * U[1], W[2] * U[0] - W[0] * U[2], W[0] * U[1] - W[1] * U[0]};
    const float uv[3] = {U[1] * V[2] - U[2] * V[1], U[2] * V[0] - U[0] * V[2], U[0] * V[1] - U[1] * V[0]};
    r.D = U[0] * vw[0] + U[1] * vw[1] + U[2] * vw[2];
    r.g = (c[0] * uv[0] + c[1] * uv[1] + c[2] * uv[2]) / r.D;
    r.dx = ((c[0] * vw[0] + c[1] * vw[1] + c[2] * vw[2]) / r.D) / r.g;
    r.dy = ((c[0] * wu[0] + c[1] * wu[1] + c[2] * wu[2]) / r.D) / r.g;
    return r;
}

// Returns false (and writes nothing) when the point does not land inside the image.
SPC_CS_HD bool camera_splat(const float* eye, const float* U, const float* V, const float* W, int width, int height,
                            const float* point, float& dx, float& dy, int& px, int& py, float& weight) {
    const CameraProjection pr = camera_project(eye, U, V, W, point);
    const float* c = pr.c;
    const float D = pr.D, g = pr.g;
    if (!(g > 0.0f)) return false;
    const float x = pr.dx, y = pr.dy;
    if (!(fabsf(x) < 1.0f && fabsf(y) < 1.0f)) return false;
    // (x + 1) may round up to 2 for x just below 1: the pixel index is clamped into the image
    int ix = (int)floorf((x + 1.0f) * 0.5f * (float)width), iy = (int)floorf((y + 1.0f) * 0.5f * (float)height);
    ix = ix < 0 ? 0 : (ix > width - 1 ? width - 1 : ix);
    iy = iy < 0 ? 0 : (iy > height - 1 ? height - 1 : iy);
    const float q[3] = {c[0] / g, c[1] / g, c[2] / g};
    const float r = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    const float we = (float)width * (float)height * (r * r * r) / (4.0f * fabsf(D));
    dx = x; dy = y; px = ix; py = iy; weight = we;
    return true;
}

}  // namespace spc
