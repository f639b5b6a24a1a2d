// Device side of the thin-lens camera (camera_lens.h): the ray generation k_spcbpt_lens, k_pt_lens and spcbpt_debug_lens_rays share.
#pragma once
#include "camera_lens.h"
#include "device_lib.h"

namespace spc {

// camera_ray (device_lib.h) with a lens: the same seed and the same jitter draws (none at subframe 0), then two draws for the lens
// point -- at subframe 0 too -- and the path goes on from that seed.  The lens axes p.lens_u / p.lens_v are the host's (camera_lens_axes);
// with radius 0 they are zero and this is camera_ray's direction scaled by the focus and normalised, from the eye: the launchers keep
// the pinhole kernels then.
SPC_DEV f3 camera_ray_lens(const KParams& p, uint32_t x, uint32_t y, uint32_t& seed, uint32_t subframe, f3& origin) {
    seed = tea4(y * p.width + x, subframe);
    float jx = 0.5f, jy = 0.5f;
    if (subframe != 0) { jx = rnd(seed); jy = rnd(seed); }
    const float u1 = rnd(seed);
    const float u2 = rnd(seed);
    float o[3], d[3];
    camera_lens_ray_axes(p.eye, p.U, p.V, p.W, (int)p.width, (int)p.height, (int)x, (int)y, jx, jy, u1, u2, p.lens_u, p.lens_v, p.lens_focus, o, d);
    origin = mk3(o[0], o[1], o[2]);
    return mk3(d[0], d[1], d[2]);
}

}  // namespace spc
