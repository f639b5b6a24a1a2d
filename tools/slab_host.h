// The slab test of one quantised child slot of a 4-wide node (layout.h) with the very arithmetic of the device (dev_traversal.h: slab4q,
// slab1q): the scale exponent from its byte, plane distance = fmaf(q, 2^e * inv, fmaf(org, inv, -(o * inv))), the near / far byte picked
// by the sign of inv, entry <= exit * 1.0000004f.  For host programs (tools/bvh_eval.cpp, tests/native/lbvh_check.cpp); build them with
// -ffp-contract=off, so that nothing but the fmaf calls below is fused.  The device takes inv with v_rcp_f32 (1 ulp): slab_inv gives the
// rounded quotient, and a caller that wants the neighbours moves it with nextafterf.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

namespace slab_host {

// safe_inv of dev_traversal.h with the IEEE quotient in the reciprocal's place
inline float slab_inv(float d) {
    const float tiny = 1e-20f;
    return 1.0f / (std::fabs(d) > tiny ? d : std::copysign(tiny, d));
}

struct Ray {
    float inv[3], ood[3];
    Ray(const float o[3], const float inv_[3]) {
        for (int k = 0; k < 3; k++) { inv[k] = inv_[k]; ood[k] = o[k] * inv_[k]; }
    }
};

// slot `i` of node record `w` (16 words) over (tmin, tmax); *entry = the entry distance the device sorts by
inline bool slot_hit(const uint32_t w[16], int i, const Ray& r, float tmin, float tmax, float* entry = nullptr) {
    float tn[3], tf[3];
    for (int k = 0; k < 3; k++) {
        float org, sc;
        memcpy(&org, &w[k], 4);
        const uint32_t e = ((w[3] >> (8 * k)) & 0xffu) << 23;
        memcpy(&sc, &e, 4);
        const float a = sc * r.inv[k];
        const float b = std::fmaf(org, r.inv[k], -r.ood[k]);
        const float lo = (float)((w[4 + k] >> (8 * i)) & 0xffu), hi = (float)((w[7 + k] >> (8 * i)) & 0xffu);
        const bool s = r.inv[k] < 0.0f;
        tn[k] = std::fmaf(s ? hi : lo, a, b);
        tf[k] = std::fmaf(s ? lo : hi, a, b);
    }
    const float t0 = std::fmax(std::fmax(tn[0], tn[1]), std::fmax(tn[2], tmin));
    const float t1 = std::fmin(std::fmin(tf[0], tf[1]), std::fmin(tf[2], tmax));
    if (entry) *entry = t0;
    return t0 <= t1 * 1.0000004f;
}

}  // namespace slab_host
