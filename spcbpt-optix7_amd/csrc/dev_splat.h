// Device helpers of the light-tracing estimator "lt" (kernels_splat.hip): a vertex of the light-vertex cache connected straight to
// the camera (BDPT strategy t = 1) and splatted onto the film.  Not part of the eye megakernel's sources: kernels.hip does not
// include this header, and the kernels here take a parameter block of their own (SplatParams), so KParams and the timed kernels'
// code stay as they are.
#pragma once
#include "camera_lens.h"
#include "camera_splat.h"
#include "device_lib.h"

namespace spc {

struct SplatParams {  // passed by value as the kernel argument block of the kernels of kernels_splat.hip
    DeviceScene scene;
    float eye[3], U[3], V[3], W[3];
    uint32_t width, height, subframe;
    int32_t row_begin, row_end, row_step;  // 8-row bands, as spcbpt_launch defines them
    const LightVertex* lvc;                // the cache of the sampler set an eye launch would read
    const int32_t* sampler_counts;         // [0] vertex_count, [1] path_count (device-resident)
    int32_t capacity;                      // vertices `lvc` holds: the device's count is never trusted beyond it
    float* splat;                          // float4 per pixel, zeroed before the launch; rgb accumulate, w unused
    float* result;                         // float4 per pixel: this subframe's radiance, merged by k_film_merge
    uint32_t* spill;                       // per-thread traversal stack overflow area
    int32_t spill_entries;
    uint32_t* diag;
    // the ordered mode (spcbpt_set_splat_order; null / 0 in the atomic mode): k_lt_records fills slot i of `records`, `keys` and
    // `vals` for every i in [0, bound); a stable sort of (keys, vals) over `bound` items leaves keys_sorted / vals_sorted for k_lt_gather
    float4* records;                       // per cache slot: (rgb, the bits of the pixel index or of the pad key width * height)
    uint32_t* keys;                        // per cache slot: the pixel index, or the pad key
    uint32_t* vals;                        // per cache slot: i
    const uint32_t* keys_sorted;
    const uint32_t* vals_sorted;
    int32_t bound;                         // host-known upper bound of min(sampler_counts[0], capacity), <= capacity
    // thin-lens camera (spcbpt_set_lens; appended): the LENS forms of the kernels only -- the host launches them when lens_radius > 0
    float lens_radius, lens_focus;
    float lens_u[3], lens_v[3];            // the lens axes (camera_lens_axes), as in KParams
};

// is row y one of the launch's rows? (lane_pixel / tile_pixel of eye_walk.h enumerate exactly these)
SPC_DEV bool splat_row_selected(const SplatParams& p, int y) {
    if (y < p.row_begin || y >= p.row_end || y >= (int)p.height) return false;
    return ((y / 8 - p.row_begin / 8) % p.row_step) == 0;
}

struct SplatJob {
    f3 origin, dir;   // shadow ray from the vertex towards the eye
    float tmax;
    f3 contrib;
    uint32_t pixel;   // y * width + x
    uint32_t index;   // the vertex's slot in the cache (set by k_lt_records, which has to know where a record goes; splat_cull leaves it)
};

// One cache vertex against the camera.  False = the vertex contributes nothing whatever the visibility (behind the camera, outside
// the image or the launch's rows, facing away, without flux or with a zero BSDF value towards the eye, or a contribution that is
// not finite); true = `job` holds its shadow ray and what to add when the ray is clear:
//   contrib = (flux / pdf) fb |n . toCam| / |c|^2  We / path_count,  fb = the light-side factor of connect_vertices (dev_rmis.h)
// No clamp (the eye kernels' ISINVALIDVALUE cut at 100 000 would bias a pure estimator); non-finite values are dropped.
// LENS (camera_lens.h): the vertex of cache slot `slot` draws a lens point O of its own -- seed tea4(slot, subframe), two numbers, so the
// draw is a function of the slot and the subframe alone, whatever thread looks at it -- and O stands where the eye stands in the pinhole
// form: the projection goes through O onto the plane in focus, and toCam, |c|^2, the cosine and the shadow ray end at O.  One lens sample
// per vertex is unbiased: the lens density 1 / area cancels against the 1 / area of the film's mean over the lens.
template <bool LENS>
SPC_DEV bool splat_cull(const SplatParams& p, const LightVertex& b, uint32_t slot, float path_count, SplatJob& job) {
    if (b.pad & SPCBPT_LV_DIRECTION) return false;   // a sky direction has no position (the host refuses "lt" with an environment map)
    const f3 bflux = ld3(b.flux);
    if (bflux.x == 0.0f && bflux.y == 0.0f && bflux.z == 0.0f) return false;
    float dx, dy, we;
    int px, py;
    f3 cam = ld3(p.eye);
    if (LENS) {
        uint32_t seed = tea4(slot, p.subframe);
        const float u1 = rnd(seed);
        const float u2 = rnd(seed);
        float off[3];
        camera_lens_point(p.lens_u, p.lens_v, u1, u2, off);
        if (!camera_splat_lens_at(p.eye, p.U, p.V, p.W, (int)p.width, (int)p.height, b.position, off, p.lens_focus, dx, dy, px, py, we)) return false;
        cam = mk3(p.eye[0] + off[0], p.eye[1] + off[1], p.eye[2] + off[2]);   // (O as camera_splat_lens_at forms it)
    }
    else if (!camera_splat(p.eye, p.U, p.V, p.W, (int)p.width, (int)p.height, b.position, dx, dy, px, py, we)) return false;
    if (!splat_row_selected(p, py)) return false;
    const f3 bpos = ld3(b.position), bn = ld3(b.normal);
    const f3 bias = cam - bpos;                   // the shadow ray of k_pt: visA = vertex, visB = eye (LENS: the lens point)
    const float r2 = dot(bias, bias);
    const float len = sqrtf(r2);
    const f3 toCam = bias / len;
    const float cosb = dot(bn, toCam);
    if (!(cosb > 0.0f)) return false;             // null_connection: the vertex faces away (an emitter is one-sided)
    f3 fb = mk3(1.0f);
    if (b.depth != 0) {
        if ((uint32_t)b.material_id >= (uint32_t)p.scene.n_mats) return false;   // (a caller-assembled cache: never an index unchecked)
        const Pbr mat_b = load_pbr_colored(p.scene, b.material_id, ld3(b.color));
        const f3 LB_DIR = normalize(ld3(b.last_position) - bpos);
        fb = brdf_div(mat_b, bsdf_eval(mat_b, bn, toCam, LB_DIR), bn, toCam);
        if (fb.x == 0.0f && fb.y == 0.0f && fb.z == 0.0f) return false;
    }
    const f3 c = (bflux / b.pdf) * fb * (fabsf(cosb) / r2 * we / path_count);
    if (!(isfinite(c.x) && isfinite(c.y) && isfinite(c.z))) return false;
    job.origin = bpos; job.dir = toCam; job.tmax = len - kEps;
    job.contrib = c;
    job.pixel = (uint32_t)py * p.width + (uint32_t)px;
    return true;
}

}  // namespace spc
