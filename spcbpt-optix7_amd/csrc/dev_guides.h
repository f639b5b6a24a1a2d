// Device helpers of the reflected-guide pass (kernels_guides.hip): albedo, normal and depth of the first surface that is not
// mirror-like along the primary ray's chain of mirror reflections -- the guides a denoiser takes when a mirror should show what it
// reflects and not its own flat albedo.  The per-bounce arithmetic is guide_step.h's, shared with the host.  Like dev_features.h this
// is not part of the eye megakernel's sources: kernels.hip does not include it, and the kernel takes a parameter block of its own
// (GuideParams), so KParams and the timed kernels' code stay as they are.
#pragma once
#include "dev_features.h"
#include "guide_step.h"

namespace spc {

struct GuideParams {  // passed by value as the kernel argument block of k_guides
    DeviceScene scene;
    float eye[3], U[3], V[3], W[3];
    uint32_t width, height, subframe;
    int32_t row_begin, row_end, row_step;  // 8-row bands, as spcbpt_launch defines them
    int32_t max_bounces;                   // 0 .. 8 mirrors followed
    float roughness_max, metallic_min;     // a surface is followed iff roughness <= roughness_max && metallic >= metallic_min
    float* albedo;                         // float4 per pixel: running mean of (throughput x base colour, coverage)
    float* normal_depth;                   // float4 per pixel: running mean of (unfolded normal, unfolded path length)
    uint32_t* spill;                       // per-thread traversal stack overflow area
    int32_t spill_entries;
    uint32_t* diag;
};

// The state a lane carries along its chain: the product of the tints, the unfolded length, the running composition M of the
// reflections (row-major; guide_step.h) and the last mirror's own unfolded normal, which a later segment's miss falls back to.
struct GuideChain {
    f3 throughput;
    float length;
    float M[9];
    f3 mirror_n;
    int bounces;
};

SPC_DEV f3 guide_unfolded(const GuideChain& c, f3 n) {
    if (c.bounces == 0) return n;   // no mirror yet: the first-hit plane's bits
    const float v[3] = {n.x, n.y, n.z};
    float o[3];
    guide_unfold(c.M, v, o);
    return mk3(o[0], o[1], o[2]);
}

// One segment of the chain: what the ray (origin, dir) of a lane with state `c` found (h valid if `hit`).  Returns true if the chain
// goes on -- `origin`, `dir` and `c` are then those of the next segment -- and false with the pixel-sample in `s` otherwise:
//   miss, primary ray         feature_sample's miss: albedo (1, 1, 1), coverage 0, normal 0, depth 0
//   miss, later segment       what the last mirror shows of the sky or the void: the throughput (that mirror's tint included),
//                             coverage 1, that mirror's normal unfolded through the mirrors before it, the length up to it
//   emitter, front            the throughput, coverage 1, the light's normal unfolded, length + t
//   emitter, back             as a miss of this segment
//   followed surface          (bounces left) throughput x tint, length + t, the mirror joins M, on along R
//   any other surface         throughput x base colour, coverage 1, N unfolded, length + t
SPC_DEV bool guide_segment(const DeviceScene& S, const GuideParams& p, bool hit, const HitRec& h, f3& origin, f3& dir, GuideChain& c,
                           FeatureSample& s) {
    s.albedo = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    s.normal_depth = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool miss = !hit;
    Geom g;
    Pbr pbr;
    f3 ln = mk3(0.0f);
    if (hit) {
        g = local_geometry(S, h);
        pbr = load_pbr(S, g.mat);
        if (g.emitter) {
            const DLight& L = S.lights[pbr.light_id];
            ln = L.type == 2 ? g.N : ld3(L.normal);   // area_light_at_hit's normal
            if (dot(dir, ln) > 0) miss = true;
        }
    }
    if (miss) {
        if (c.bounces > 0) {
            s.albedo = make_float4(c.throughput.x, c.throughput.y, c.throughput.z, 1.0f);
            s.normal_depth = make_float4(c.mirror_n.x, c.mirror_n.y, c.mirror_n.z, c.length);
        }
        return false;
    }
    if (g.emitter) {
        const f3 n = guide_unfolded(c, ln);
        s.albedo = make_float4(c.throughput.x, c.throughput.y, c.throughput.z, 1.0f);
        s.normal_depth = make_float4(n.x, n.y, n.z, c.length + h.t);
        return false;
    }
    Counts<false> cn;
    color_tex_sample(S, g, pbr, cn);
    f3 N = g.N;
    if (dot(N, dir) > 0.f) N = -N;
    if (c.bounces < p.max_bounces && guide_followed(pbr.roughness, pbr.metallic, p.roughness_max, p.metallic_min)) {
        const float Nv[3] = {N.x, N.y, N.z}, dv[3] = {dir.x, dir.y, dir.z}, base[3] = {pbr.base.x, pbr.base.y, pbr.base.z};
        float tint[3], R[3];
        guide_tint(base, pbr.metallic, pbr.specular, pbr.specularTint, dot(N, dir), tint);
        guide_reflect(dv, Nv, R);
        c.mirror_n = guide_unfolded(c, N);
        guide_compose(c.M, Nv);
        c.throughput = c.throughput * mk3(tint[0], tint[1], tint[2]);
        c.length = c.length + h.t;
        c.bounces += 1;
        origin = g.P;
        dir = mk3(R[0], R[1], R[2]);
        return true;
    }
    const f3 n = guide_unfolded(c, N);
    const f3 a = c.throughput * pbr.base;
    s.albedo = make_float4(a.x, a.y, a.z, 1.0f);
    s.normal_depth = make_float4(n.x, n.y, n.z, c.length + h.t);
    return false;
}

}  // namespace spc
