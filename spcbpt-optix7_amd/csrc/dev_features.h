// Device helpers of the first-hit feature pass (kernels_features.hip): albedo, geometric normal and depth of the primary ray's hit,
// the guides every image-space denoiser takes.  Not part of the eye megakernel's sources: kernels.hip does not include this header,
// and the kernel takes a parameter block of its own (FeatureParams), so KParams and the timed kernels' code stay as they are.
#pragma once
#include "device_lib.h"

namespace spc {

struct FeatureParams {  // passed by value as the kernel argument block of k_features
    DeviceScene scene;
    float eye[3], U[3], V[3], W[3];
    uint32_t width, height, subframe;
    int32_t row_begin, row_end, row_step;  // 8-row bands, as spcbpt_launch defines them
    float* albedo;                         // float4 per pixel: running mean of (base colour, coverage)
    float* normal_depth;                   // float4 per pixel: running mean of (face-forwarded geometric normal, hit distance)
    uint32_t* spill;                       // per-thread traversal stack overflow area
    int32_t spill_entries;
    uint32_t* diag;
};

struct FeatureSample { float4 albedo, normal_depth; };

// What the primary ray `dir` of k_pt sees first (h valid if `hit`), as this subframe's sample:
//   surface          base colour after color_tex_sample, coverage 1, the normal turned against the ray, the hit distance
//   emitter, front   (1, 1, 1), 1, the light's normal (a quad's own, a mesh light's triangle's), the hit distance
//   emitter, back    as a miss: path rays see an emitter from its front only
//   miss             (1, 1, 1), coverage 0, normal 0, depth 0 -- albedo 1 so that radiance / albedo needs no branch anywhere
SPC_DEV FeatureSample feature_sample(const DeviceScene& S, bool hit, const HitRec& h, f3 dir) {
    FeatureSample s;
    s.albedo = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    s.normal_depth = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!hit) return s;
    const Geom g = local_geometry(S, h);
    Pbr pbr = load_pbr(S, g.mat);
    if (g.emitter) {
        const DLight& L = S.lights[pbr.light_id];
        const f3 ln = L.type == 2 ? g.N : ld3(L.normal);   // area_light_at_hit's normal
        if (dot(dir, ln) > 0) return s;
        s.albedo.w = 1.0f;
        s.normal_depth = make_float4(ln.x, ln.y, ln.z, h.t);
        return s;
    }
    Counts<false> cn;
    color_tex_sample(S, g, pbr, cn);
    f3 N = g.N;
    if (dot(N, dir) > 0.f) N = -N;
    s.albedo = make_float4(pbr.base.x, pbr.base.y, pbr.base.z, 1.0f);
    s.normal_depth = make_float4(N.x, N.y, N.z, h.t);
    return s;
}

// running mean by subframe, the film's: lerp(prev, sample, 1 / (subframe + 1)); subframe 0 overwrites
SPC_DEV float4 feature_mean(float4 prev, float4 s, float a) {
    return make_float4(lerpf(prev.x, s.x, a), lerpf(prev.y, s.y, a), lerpf(prev.z, s.z, a), lerpf(prev.w, s.w, a));
}

}  // namespace spc
