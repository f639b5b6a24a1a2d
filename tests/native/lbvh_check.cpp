// Host-side structural check of the BVH builders (csrc/lbvh.cpp): every triangle sits in exactly one leaf, every slot box
// contains what hangs below it, empty slots are point boxes at 1e30.  Usage: lbvh_check <n_triangles> <seed>   (a seeded cloud)
//                                                                            lbvh_check mesh <file> [rays]   (a mesh: int32 nv, nt;
// float32 vertices[nv][3]; uint32 indices[nt][3] -- the format of tools/bvh_eval.cpp; tests/hard_scenes.py writes its scenes so).
// On a mesh the program also runs the DEVICE-ARITHMETIC PATH CHECK: for seeded rays and every triangle that is a clear hit in double
// (the definition of tests/ray_verdict.py, K = 64, KT = 16, no culling), every slot on the way from the root to the triangle's leaf
// must pass the slab test as the device evaluates it (tools/slab_host.h), over the ray's interval and over (tmin, t + tt), with the
// reciprocal direction rounded and one ulp either side of that (v_rcp_f32 is good to 1 ulp).  Build with -ffp-contract=off.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <random>
#include <vector>

#include "../../spcbpt-optix7_amd/csrc/lbvh.cpp"
#include "../../tools/slab_host.h"

using namespace spc;

struct Check {
    const Lbvh& b;
    std::vector<int> seen;
    long long leaves = 0, nodes = 0;
    double sah = 0, slack = 0;
    int bad = 0;
    bool ok = true;
    explicit Check(const Lbvh& l) : b(l), seen(l.tri_orig.size(), 0) {}
    static int geti(const float* p) { int v; memcpy(&v, p, 4); return v; }
    // returns the box of everything below `node`; checks that every decoded (quantised) slot box contains its subtree
    void walk(int node, float lo[3], float hi[3], int depth) {
        nodes++;
        if (depth > 200) { ok = false; return; }
        uint32_t w[16];
        memcpy(w, &b.nodes[(size_t)node * 16], sizeof(w));
        float org[3]; memcpy(org, w, 12);
        float sc[3];
        for (int k = 0; k < 3; k++) { const uint32_t e = ((w[3] >> (8 * k)) & 0xffu) << 23; memcpy(&sc[k], &e, 4); }
        const uint32_t qlo[3] = {w[4], w[5], w[6]}, qhi[3] = {w[7], w[8], w[9]};
        const uint32_t refs[4] = {w[10], w[11], w[12], w[13]};
        for (int k = 0; k < 3; k++) { lo[k] = 1e30f; hi[k] = -1e30f; }
        bool seen_empty = false;
        for (int i = 0; i < 4; i++) {
            const uint32_t ref = refs[i];
            if (ref == 0x80000000u) {
                seen_empty = true;
                for (int k = 0; k < 3; k++) if (((qlo[k] >> (8 * i)) & 0xffu) != 255u || ((qhi[k] >> (8 * i)) & 0xffu) != 0u) ok = false;
                continue;
            }
            if (seen_empty) ok = false;  // used slots come first
            float slo[3], shi[3];
            for (int k = 0; k < 3; k++) {
                slo[k] = org[k] + (float)((qlo[k] >> (8 * i)) & 0xffu) * sc[k];
                shi[k] = org[k] + (float)((qhi[k] >> (8 * i)) & 0xffu) * sc[k];
            }
            float clo[3], chi[3];
            int cnt = 1;
            if (ref & 0x80000000u) {
                const int first = (int)((ref & 0x7fffffffu) >> 3);
                cnt = (int)(ref & 7u);
                if (cnt < 1 || cnt > 4) ok = false;
                for (int k = 0; k < 3; k++) { clo[k] = 1e30f; chi[k] = -1e30f; }
                for (int t = first; t < first + cnt; t++) {
                    if (t < 0 || t >= (int)seen.size()) { ok = false; continue; }
                    seen[t]++;
                    const float* tr = &b.tris[(size_t)t * 16];
                    for (int v = 0; v < 3; v++) for (int k = 0; k < 3; k++) { clo[k] = std::min(clo[k], tr[4 * v + k]); chi[k] = std::max(chi[k], tr[4 * v + k]); }
                }
                leaves++;
            } else {
                if ((int)ref <= node || (size_t)ref * 16 >= b.nodes.size()) { ok = false; continue; }
                walk((int)ref, clo, chi, depth + 1);
            }
            for (int k = 0; k < 3; k++) {
                if (clo[k] < slo[k] || chi[k] > shi[k]) { ok = false; if (bad++ < 5) printf("node %d slot %d axis %d: [%g,%g] not in [%g,%g]\n", node, i, k, clo[k], chi[k], slo[k], shi[k]); }
                lo[k] = std::min(lo[k], clo[k]); hi[k] = std::max(hi[k], chi[k]);
                slack += (shi[k] - slo[k]) - (chi[k] - clo[k]);
            }
            const float dx = shi[0] - slo[0], dy = shi[1] - slo[1], dz = shi[2] - slo[2];
            sah += (double)(dx * dy + dy * dz + dz * dx) * cnt;
        }
    }
};

static void generate_cloud(int n, unsigned seed, std::vector<float>& V, std::vector<uint32_t>& I, std::vector<int32_t>& M, std::vector<uint8_t>& E, int& n_quads) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> U(0.0f, 1.0f);
    for (int t = 0; t < n; t++) {
        // clustered small triangles plus a few large ones and exact duplicates (coincident centroids)
        float c[3] = {U(rng) * 10, U(rng) * 3, U(rng) * 10};
        float s = (t % 97 == 0) ? 3.0f : 0.05f;
        if (t % 50 == 1 && t > 0) { for (int k = 0; k < 9; k++) V.push_back(V[V.size() - 9]); }
        else if (t % 5 == 2 && t > 0) {   // the second half of a quad: (P0, P2 of the triangle before, a new corner) -- a fan pair (lbvh.h)
            const size_t a = V.size() - 9;
            for (int k = 0; k < 3; k++) V.push_back(V[a + k]);
            for (int k = 0; k < 3; k++) V.push_back(V[a + 6 + k]);
            for (int k = 0; k < 3; k++) V.push_back(V[a + k] + V[a + 6 + k] - V[a + 3 + k]);
            n_quads++;
        }
        else for (int v = 0; v < 3; v++) for (int k = 0; k < 3; k++) V.push_back(c[k] + s * (U(rng) - 0.5f));
        for (int v = 0; v < 3; v++) I.push_back(3 * t + v);
        M.push_back(0); E.push_back((uint8_t)(t % 5 == 2 || t % 5 == 1 ? (t / 5) % 2 : 0));
    }
}


// ---- the device-arithmetic path check ------------------------------------------------------------------------------------------------
struct D3 { double x, y, z; };
static D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static D3 operator*(D3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
static double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static double len(D3 a) { return std::sqrt(dot(a, a)); }

// tests/ray_verdict.py's clear hit of ray (o, d) over (tmin, tmax) on triangle P (no culling); t and tt are returned
static bool clear_hit(const D3 P[3], D3 o, D3 d, double tmin, double tmax, double ext, double& t, double& tt) {
    const double EPS = std::ldexp(1.0, -24), K = 64.0, KT = 16.0, COS_MIN = 1e-4, T_REL = 1e-5;
    const D3 e1 = P[1] - P[0], e2 = P[2] - P[0], n = cross(e1, e2);
    const double nl = len(n);
    if (!(nl > 0.0)) return false;   // a zero-area triangle is never a hit
    const D3 nh = n * (1.0 / nl);
    const double sinphi = nl / (len(e1) * len(e2)), dl = len(d), dn = dot(d, nh);
    t = dot(P[0] - o, nh) / dn;
    const double ac = std::fabs(dn / dl);
    if (!(ac > COS_MIN) || !std::isfinite(t)) return false;
    const D3 h = o + d * t;
    double dist = 1e300;
    for (int k = 0; k < 3; k++) {
        const D3 A = P[k], B = P[(k + 1) % 3];
        D3 ed = B - A; ed = ed * (1.0 / len(ed));
        dist = std::min(dist, dot(h - A, cross(nh, ed)));
    }
    const double omax = std::max(std::fabs(o.x), std::max(std::fabs(o.y), std::fabs(o.z)));
    const double dw = K * EPS * (ext + omax + std::fabs(t) * dl);
    tt = std::max(T_REL * std::max(1.0, std::fabs(t)), KT * EPS * (len(o - P[0]) + ext) / (sinphi * ac * dl));
    return dist * ac > dw && t > tmin + tt && t < tmax - tt;
}

struct PathCheck {
    const Lbvh& b;
    std::vector<int> parent_node, parent_slot;   // of every node
    std::vector<int> leaf_node, leaf_slot;       // of every triangle record
    long long pairs = 0, slots = 0, culled = 0;
    explicit PathCheck(const Lbvh& l) : b(l) {
        const int n_nodes = (int)(b.nodes.size() / 16), n = (int)b.tri_orig.size();
        parent_node.assign(n_nodes, -1); parent_slot.assign(n_nodes, -1); leaf_node.assign(n, -1); leaf_slot.assign(n, -1);
        for (int node = 0; node < n_nodes; node++)
            for (int i = 0; i < 4; i++) {
                uint32_t ref; memcpy(&ref, &b.nodes[(size_t)node * 16 + 10 + i], 4);
                if (ref == 0x80000000u) continue;
                if (ref & 0x80000000u) { for (uint32_t t = (ref & 0x7fffffffu) >> 3, e = t + (ref & 7u); t < e && t < (uint32_t)n; t++) { leaf_node[t] = node; leaf_slot[t] = i; } }
                else if ((int)ref < n_nodes) { parent_node[ref] = node; parent_slot[ref] = i; }
            }
    }
    // one ray against every triangle record
    void ray(const float o[3], const float d[3], float tmin, float tmax, double ext) {
        const int n = (int)b.tri_orig.size();
        const D3 od{o[0], o[1], o[2]}, dd{d[0], d[1], d[2]};
        for (int t = 0; t < n; t++) {
            const float* q = &b.tris[(size_t)t * 16];
            const D3 P[3] = {{q[0], q[1], q[2]}, {q[4], q[5], q[6]}, {q[8], q[9], q[10]}};
            double th, tt;
            if (!clear_hit(P, od, dd, tmin, tmax, ext, th, tt)) continue;
            pairs++;
            const float narrowed = std::nextafterf((float)(th + tt), INFINITY);   // `best` after a hit that the verdict still calls a tie
            for (int ulp = -1; ulp <= 1; ulp++) {
                float inv[3];
                for (int k = 0; k < 3; k++) {
                    inv[k] = slab_host::slab_inv(d[k]);
                    if (ulp) inv[k] = std::nextafterf(inv[k], (ulp > 0) == (inv[k] > 0) ? INFINITY : -INFINITY);   // one ulp larger / smaller in magnitude
                }
                const slab_host::Ray r(o, inv);
                for (int node = leaf_node[t], slot = leaf_slot[t]; node >= 0; slot = parent_slot[node], node = parent_node[node]) {
                    uint32_t w[16]; memcpy(w, &b.nodes[(size_t)node * 16], 64);
                    for (int iv = 0; iv < 2; iv++) {
                        slots++;
                        float entry;
                        if (!slab_host::slot_hit(w, slot, r, tmin, iv ? narrowed : tmax, &entry)) {
                            if (culled++ < 5)
                                printf("culled: record %d (triangle %d) t=%.9g tt=%.3g, node %d slot %d, rcp %+d ulp, interval %s, entry %.9g; ray o=(%.9g %.9g %.9g) d=(%.9g %.9g %.9g)\n",
                                       t, b.tri_orig[t], th, tt, node, slot, ulp, iv ? "(tmin, t + tt)" : "own", entry, o[0], o[1], o[2], d[0], d[1], d[2]);
                        }
                    }
                    if (node == 0) break;
                }
            }
        }
    }
};

// seeded rays for the path check: from the grown box at a random interior point of a random triangle, from the box in a random
// direction, from 50 units outside at an interior point, along an axis, and from one interior point towards another
static void path_check(const Lbvh& out, int n_rays, unsigned seed, PathCheck& pc) {
    const int n = (int)out.tri_orig.size();
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, ext = 0;
    for (int t = 0; t < n; t++) for (int v = 0; v < 3; v++) for (int k = 0; k < 3; k++) {
        const double x = out.tris[(size_t)t * 16 + 4 * v + k];
        lo[k] = std::min(lo[k], x); hi[k] = std::max(hi[k], x); ext = std::max(ext, std::fabs(x));
    }
    for (int k = 0; k < 3; k++) { const double g = std::max(0.0, 1.0 - (hi[k] - lo[k])) * 0.5; lo[k] -= g; hi[k] += g; }
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> G(0.0, 1.0);
    auto interior = [&](double p[3]) {
        const float* q = &out.tris[(size_t)(rng() % (uint64_t)n) * 16];
        double a = U(rng), b = U(rng);
        if (a + b > 1) { a = 1 - a; b = 1 - b; }
        for (int k = 0; k < 3; k++) p[k] = (double)q[k] * (1 - a - b) + (double)q[4 + k] * a + (double)q[8 + k] * b;
    };
    for (int i = 0; i < n_rays; i++) {
        double o[3], d[3], p[3];
        for (int k = 0; k < 3; k++) o[k] = lo[k] + U(rng) * (hi[k] - lo[k]);
        const int kind = i % 5;
        if (kind == 1) for (int k = 0; k < 3; k++) d[k] = G(rng);
        else if (kind == 3) { for (int k = 0; k < 3; k++) d[k] = 0.0; d[rng() % 3] = (rng() & 1) ? 1.0 : -1.0; }
        else {
            if (kind == 2) { double g[3] = {G(rng), G(rng), G(rng)}; const double l = std::sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]); for (int k = 0; k < 3; k++) o[k] = 0.5 * (lo[k] + hi[k]) + 50.0 * g[k] / l; }
            if (kind == 4) { interior(o); }
            float of[3] = {(float)o[0], (float)o[1], (float)o[2]};
            interior(p);
            for (int k = 0; k < 3; k++) d[k] = p[k] - (double)of[k];
        }
        const double l = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (!(l > 1e-6)) continue;
        const float of[3] = {(float)o[0], (float)o[1], (float)o[2]}, df[3] = {(float)(d[0] / l), (float)(d[1] / l), (float)(d[2] / l)};
        pc.ray(of, df, 1e-3f, 1e16f, ext);
    }
}

static bool load_mesh(const char* path, std::vector<float>& V, int& n) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    int hdr[2];
    if (fread(hdr, 4, 2, f) != 2 || hdr[0] < 3 || hdr[1] < 1 || hdr[0] > (1 << 24) || hdr[1] > (1 << 24)) { fclose(f); return false; }
    std::vector<float> vin((size_t)3 * hdr[0]);
    std::vector<uint32_t> iin((size_t)3 * hdr[1]);
    const bool ok = fread(vin.data(), 4, vin.size(), f) == vin.size() && fread(iin.data(), 4, iin.size(), f) == iin.size();
    fclose(f);
    if (!ok) return false;
    n = hdr[1];
    V.clear();
    for (uint32_t ix : iin) { if (ix >= (uint32_t)hdr[0]) return false; for (int k = 0; k < 3; k++) V.push_back(vin[3 * (size_t)ix + k]); }   // one corner set per triangle, as the cloud below
    return true;
}

int main(int argc, char** argv) {
    const bool from_mesh = argc > 2 && strcmp(argv[1], "mesh") == 0;
    int n = !from_mesh && argc > 1 ? atoi(argv[1]) : 20000;
    const unsigned seed = !from_mesh && argc > 2 ? (unsigned)atoi(argv[2]) : 1u;
    std::vector<float> V; std::vector<uint32_t> I; std::vector<int32_t> M; std::vector<uint8_t> E;
    int n_quads = 0;
    if (from_mesh) {
        if (!load_mesh(argv[2], V, n)) { fprintf(stderr, "cannot read mesh %s\n", argv[2]); return 2; }
        for (int t = 0; t < n; t++) { for (int v = 0; v < 3; v++) I.push_back(3 * t + v); M.push_back(0); E.push_back(0); }
    } else {
        generate_cloud(n, seed, V, I, M, E, n_quads);
    }
    HostMesh m; m.vertices = V.data(); m.indices = I.data(); m.tri_material = M.data(); m.tri_emitter = E.data();
    m.n_vertices = 3 * n; m.n_triangles = n;
    Lbvh out;
    auto t0 = std::chrono::steady_clock::now();
    build_lbvh(m, out);
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    Check c(out);
    float lo[3], hi[3];
    c.walk(0, lo, hi, 1);
    for (int s : c.seen) if (s != 1) c.ok = false;
    std::vector<int> perm(out.tri_orig.begin(), out.tri_orig.end());
    std::sort(perm.begin(), perm.end());
    for (int i = 0; i < n; i++) if (perm[i] != i) c.ok = false;
    int n_flat = 0;
    // the triangle records still belong to the triangles tri_orig names (make_fan_pairs reorders inside leaves) ...
    for (int i = 0; i < n; i++) {
        const float* tr = &out.tris[(size_t)i * 16];
        const float* src = &V[(size_t)9 * out.tri_orig[i]];
        // (a triangle without area has P0 for all three corners of its record: lbvh.cpp, zero_area)
        const bool flat = zero_area(src, src + 3, src + 6);
        n_flat += flat;
        for (int v = 0; v < 3; v++) if (memcmp(tr + 4 * v, src + (flat ? 0 : 3 * v), 12) != 0) { c.ok = false; printf("record %d is not triangle %d\n", i, out.tri_orig[i]); break; }
    }
    // ... and the pair slots (lbvh.h: Lbvh::pairs): a slot flagged "pair" holds (A.P0, A.P1 - A.P0, A.P2 - A.P0, B.P2 - A.P0) of triangles i, i + 1 of ONE
    // leaf with B = (A.P0, A.P2, B.P2) bit for bit and both culling flags; every other slot holds its own triangle
    {
        std::vector<int> leaf_of((size_t)n, -1);
        int leaf_id = 0;
        for (size_t nd = 0; nd < out.nodes.size() / 16; nd++)
            for (int k = 0; k < 4; k++) {
                uint32_t ref; memcpy(&ref, &out.nodes[nd * 16 + 10 + k], 4);
                if (!(ref & 0x80000000u)) continue;
                for (uint32_t t = (ref & 0x7fffffffu) >> 3, e = t + (ref & 7u); t < e && t < (uint32_t)n; t++) leaf_of[t] = leaf_id;
                leaf_id++;
            }
        int pairs = 0;
        if ((int)out.pairs.size() != 16 * n) { c.ok = false; printf("pair slots: %zu floats for %d triangles\n", out.pairs.size(), n); }
        for (int i = 0; c.ok && i < n; i++) {
            const float* q = &out.pairs[(size_t)i * 16];
            const float* a = &out.tris[(size_t)i * 16];
            uint32_t fl, ma; memcpy(&fl, q + 15, 4); memcpy(&ma, a + 15, 4);
            // (the slot holds the corner P0 and the EDGES P1 - P0, P2 - P0 as FP32 differences)
            float e1[3], e2[3];
            for (int k = 0; k < 3; k++) { e1[k] = a[4 + k] - a[k]; e2[k] = a[8 + k] - a[k]; }
            bool good = memcmp(q, a, 12) == 0 && memcmp(q + 4, e1, 12) == 0 && memcmp(q + 8, e2, 12) == 0 && ((fl ^ ma) & 0x80000000u) == 0;
            if (fl & 1u) {
                pairs++;
                if (i + 1 >= n || leaf_of[i + 1] != leaf_of[i] || (i > 0 && (([&] { uint32_t p; memcpy(&p, &out.pairs[(size_t)(i - 1) * 16 + 15], 4); return p & 1u; })()))) good = false;
                else {
                    const float* b = &out.tris[(size_t)(i + 1) * 16];
                    uint32_t mb; memcpy(&mb, b + 15, 4);
                    float e3[3];
                    for (int k = 0; k < 3; k++) e3[k] = b[8 + k] - a[k];
                    good = good && memcmp(b, a, 12) == 0 && memcmp(b + 4, a + 8, 12) == 0 && memcmp(q + 12, e3, 12) == 0 && ((fl >> 30) & 1u) == (mb >> 31);
                }
            } else good = good && (fl & 0x7fffffffu) == 0;
            if (!good) { c.ok = false; printf("pair slot %d is wrong (flags %08x)\n", i, fl); }
        }
        if (out.n_paired != 2 * pairs) { c.ok = false; printf("n_paired %d, slots flagged %d\n", out.n_paired, pairs); }
        // the halves of a quad share a bounding box, so the builder rarely separates them: most of the quads made above end up paired
        if (n >= 700 && pairs * 2 < n_quads) { c.ok = false; printf("only %d of %d quads paired\n", pairs, n_quads); }
    }
    // every node is reachable exactly once (the walk counts them), and the first HOT_NODES records are the hottest-first crown of the
    // tree (lbvh.cpp: hot_nodes_first): node 0 is the root, the parent of a hot node is hot and comes before it, and no node outside
    // the crown has a larger box than the crown's last (the crown is the top of the area order, ties aside)
    const int n_nodes = (int)(out.nodes.size() / 16);
    if (c.nodes != n_nodes) { c.ok = false; printf("walk reached %lld of %d nodes\n", c.nodes, n_nodes); }
    {
        std::vector<int> parent((size_t)n_nodes, -1);
        std::vector<float> area((size_t)n_nodes, 0.0f);
        for (int node = 0; node < n_nodes; node++) {
            uint32_t w[16];
            memcpy(w, &out.nodes[(size_t)node * 16], sizeof(w));
            float org[3]; memcpy(org, w, 12);
            float sc[3];
            for (int k = 0; k < 3; k++) { const uint32_t e = ((w[3] >> (8 * k)) & 0xffu) << 23; memcpy(&sc[k], &e, 4); }
            for (int i = 0; i < 4; i++) {
                const uint32_t ref = w[10 + i];
                if (ref & 0x80000000u) continue;
                float e[3];
                for (int k = 0; k < 3; k++) e[k] = (float)((w[7 + k] >> (8 * i)) & 0xffu) * sc[k] - (float)((w[4 + k] >> (8 * i)) & 0xffu) * sc[k];
                parent[ref] = node; area[ref] = e[0] * e[1] + e[1] * e[2] + e[2] * e[0];
            }
        }
        // (round 6, advisor) areas are read from the 8-bit boxes, which are rounded outward on the PARENT's grid: a child's stored area
        // may exceed by a grid cell per axis (~1 %) what its parent measures in the grandparent's grid, so the largest-first pop order
        // of the builder is monotone only up to that slack.  The structural property (a hot node's parent is hot and precedes it) is exact.
        const float slack = 1.02f;
        const int hot = std::min(n_nodes, (int)HOT_NODES);
        for (int i = 1; i < hot; i++) {
            if (parent[i] < 0 || parent[i] >= i) { c.ok = false; printf("hot node %d: parent %d\n", i, parent[i]); }
            if (i > 1 && area[i] > area[i - 1] * slack) { c.ok = false; printf("hot node %d: area %g after %g\n", i, area[i], area[i - 1]); }
        }
        for (int i = hot; i < n_nodes && hot > 1; i++)
            if (parent[i] >= 0 && parent[i] < hot && area[i] > area[hot - 1] * slack) { c.ok = false; printf("node %d (area %g) should be in the crown (last %g)\n", i, area[i], area[hot - 1]); break; }
    }
    int root_slots = 0;
    for (int i = 0; i < 4; i++) { uint32_t ref; memcpy(&ref, &out.nodes[10 + i], 4); if (ref != 0x80000000u) root_slots++; }
    long long pairs = 0, culled = 0;
    if (from_mesh) {
        PathCheck pc(out);
        for (int t = 0; t < n; t++) if (pc.leaf_node[t] < 0) c.ok = false;
        path_check(out, argc > 3 ? atoi(argv[3]) : 2000, 7u, pc);
        pairs = pc.pairs; culled = pc.culled;
        if (culled) c.ok = false;
    }
    printf("%s n=%d nodes=%lld leaves=%lld depth=%d root_slots=%d zero_area=%d clear_pairs=%lld culled=%lld sah=%.1f build=%.3fs\n", c.ok ? "OK" : "FAIL", n, c.nodes, c.leaves,
           out.depth, root_slots, n_flat, pairs, culled, c.sah, sec);
    return c.ok ? 0 : 1;
}
