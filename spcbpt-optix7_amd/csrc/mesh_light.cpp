// Mesh lights, host side: areas, CMF, Morton patches and the guide table of one light's triangles (mesh_light.h), and the C entry
// spcbpt_mesh_light_table that hands the same table to tests and hosts without a device.
#include "mesh_light.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/spcbpt.h"

namespace spc {

static uint32_t spread10(uint32_t v) {   // 10 bits -> every third bit
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

void build_mesh_light_table(const float* vertices, const uint32_t* indices, int n_triangles, int n_patches, MeshLightTable& out) {
    out = MeshLightTable();
    std::vector<double> area((size_t)std::max(n_triangles, 0)), cen((size_t)3 * std::max(n_triangles, 0));
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    std::vector<int32_t> kept;
    for (int t = 0; t < n_triangles; t++) {
        const float* p0 = vertices + 3 * (size_t)indices[3 * (size_t)t];
        const float* p1 = vertices + 3 * (size_t)indices[3 * (size_t)t + 1];
        const float* p2 = vertices + 3 * (size_t)indices[3 * (size_t)t + 2];
        // the edges as the device holds them (float differences), their cross product in double
        const double e1[3] = {(double)(p1[0] - p0[0]), (double)(p1[1] - p0[1]), (double)(p1[2] - p0[2])};
        const double e2[3] = {(double)(p2[0] - p0[0]), (double)(p2[1] - p0[1]), (double)(p2[2] - p0[2])};
        const double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double a = 0.5 * std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        area[(size_t)t] = a;
        // (the float cross product must not vanish either: the device normalises it)
        const float e1f[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, e2f[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
        const float cf[3] = {e1f[1] * e2f[2] - e1f[2] * e2f[1], e1f[2] * e2f[0] - e1f[0] * e2f[2], e1f[0] * e2f[1] - e1f[1] * e2f[0]};
        const float lf = cf[0] * cf[0] + cf[1] * cf[1] + cf[2] * cf[2];
        if (!(a > 0.0) || !std::isfinite(a) || !(lf > 0.0f) || !std::isfinite(1.0f / std::sqrt(lf))) continue;
        kept.push_back(t);
        for (int k = 0; k < 3; k++) {
            const double m = ((double)p0[k] + (double)p1[k] + (double)p2[k]) / 3.0;
            cen[3 * (size_t)t + k] = m;
            lo[k] = std::min(lo[k], m); hi[k] = std::max(hi[k], m);
        }
    }
    if (kept.empty()) return;
    std::vector<uint32_t> code((size_t)n_triangles, 0u);
    for (int t : kept) {
        uint32_t q[3];
        for (int k = 0; k < 3; k++) {
            const double ext = hi[k] - lo[k];
            const double f = ext > 0.0 ? (cen[3 * (size_t)t + k] - lo[k]) / ext : 0.0;
            q[k] = (uint32_t)std::min(1023.0, std::max(0.0, f * 1024.0));
        }
        code[(size_t)t] = spread10(q[0]) | (spread10(q[1]) << 1) | (spread10(q[2]) << 2);
    }
    std::sort(kept.begin(), kept.end(), [&](int32_t a, int32_t b) { return code[(size_t)a] != code[(size_t)b] ? code[(size_t)a] < code[(size_t)b] : a < b; });
    double total = 0.0;
    for (int t : kept) total += area[(size_t)t];
    const int n = (int)kept.size();
    const int np = std::max(1, std::min(n_patches, n));
    out.tri = kept; out.area = total; out.n_patches = np;
    out.cmf.resize((size_t)n); out.patch.resize((size_t)n); out.tri_area.resize((size_t)n);
    double run = 0.0;
    int patch = 0;
    for (int i = 0; i < n; i++) {
        const double a = area[(size_t)kept[(size_t)i]];
        run += a;
        out.tri_area[(size_t)i] = (float)a;
        out.cmf[(size_t)i] = (float)(run / total);
        out.patch[(size_t)i] = patch;
        // the next triangle opens the next patch once this one holds its share of the area -- or when only as many triangles
        // are left as patches, so that no patch stays empty
        const int tris_left = n - 1 - i, patches_left = np - 1 - patch;
        if (patches_left > 0 && (run >= total * (double)(patch + 1) / (double)np || tris_left <= patches_left)) patch++;
    }
    out.cmf[(size_t)n - 1] = 1.0f;
    for (int i = 1; i < n; i++) out.cmf[(size_t)i] = std::max(out.cmf[(size_t)i], out.cmf[(size_t)i - 1]);   // (rounding cannot make it decrease; kept as a guarantee)
}

int mesh_light_guide_buckets(int n_entries) {
    int b = 16;
    while (b < n_entries && b < 65536) b *= 2;
    return b;
}

void build_mesh_light_guide(const std::vector<float>& cmf, int buckets, std::vector<uint32_t>& guide) {
    guide.resize((size_t)buckets);
    size_t k = 0;
    for (int b = 0; b < buckets; b++) {
        const float t = (float)b / (float)buckets;   // exact, and so is u * buckets: every u of bucket b is >= t
        while (k + 1 < cmf.size() && !(cmf[k] > t)) k++;
        guide[(size_t)b] = (uint32_t)k;
    }
}

}  // namespace spc

extern "C" int spcbpt_mesh_light_table(const float* vertices, int n_vertices, const uint32_t* indices, int n_triangles, int n_patches,
                                       int32_t* tri_out, float* cmf_out, int32_t* patch_out, float* tri_area_out, double* area_out,
                                       int* n_patches_out) {
    if (!vertices || !indices || n_vertices < 3 || n_triangles < 1 || n_patches < 1) return SPCBPT_ERR_INVALID_ARG;
    for (size_t i = 0; i < 3 * (size_t)n_triangles; i++) if (indices[i] >= (uint32_t)n_vertices) return SPCBPT_ERR_INVALID_ARG;
    spc::MeshLightTable t;
    spc::build_mesh_light_table(vertices, indices, n_triangles, n_patches, t);
    const size_t n = t.tri.size();
    if (tri_out) memcpy(tri_out, t.tri.data(), n * sizeof(int32_t));
    if (cmf_out) memcpy(cmf_out, t.cmf.data(), n * sizeof(float));
    if (patch_out) memcpy(patch_out, t.patch.data(), n * sizeof(int32_t));
    if (tri_area_out) memcpy(tri_area_out, t.tri_area.data(), n * sizeof(float));
    if (area_out) *area_out = t.area;
    if (n_patches_out) *n_patches_out = t.n_patches;
    return (int)n;
}
