// C ABI (include/spcbpt.h) over the HIP kernels: create / destroy, state, launches by name.  The host side of the reference this
// replaces is cited per function in include/spcbpt.h.  (Read-backs, counters and test hooks: capi_debug.hip; exchange: capi_exchange.hip.)
#include "capi_common.h"
#include "mesh_light.h"

using namespace spc;

static thread_local std::string g_create_error;

// spcbpt_create (ml == nullptr) and spcbpt_create_lit
static int create_context(const spcbpt_scene_desc* sc, const spcbpt_mesh_light* ml, int n_ml, int device, spcbpt_ctx** out) {
    if (!sc || !out) { g_create_error = "null argument"; return SPCBPT_ERR_INVALID_ARG; }
    *out = nullptr;
    if (!ml) {
        if (!sc->vertices || !sc->indices || !sc->tri_material || sc->n_vertices < 3 || sc->n_triangles < 1 || sc->n_materials < 1 ||
            !sc->materials || sc->n_lights < 1 || !sc->lights) {
            g_create_error = "scene needs vertices, indices, tri_material, >=1 material and >=1 quad light";
            return SPCBPT_ERR_INVALID_ARG;
        }
    } else {
        if (!sc->vertices || !sc->indices || !sc->tri_material || sc->n_vertices < 3 || sc->n_triangles < 1 || sc->n_materials < 1 ||
            !sc->materials || sc->n_lights < 0 || (sc->n_lights > 0 && !sc->lights) || n_ml < 0 || sc->n_lights + n_ml < 1) {
            g_create_error = "scene needs vertices, indices, tri_material, >=1 material and >=1 light (quad or mesh)";
            return SPCBPT_ERR_INVALID_ARG;
        }
    }
    // validate the geometry before anything reaches the builder or a kernel -- and before a device is asked for: a scene that cannot be
    // built is refused the same way with and without one.  The builder's std::min / std::max drop a NaN silently, and an infinite corner
    // leaves no finite box to quantise: non-finite coordinates (every route ends here: .scene and glTF files are loaded into a scene desc) go back.
    for (int v = 0; v < sc->n_vertices; v++)
        for (int k = 0; k < 3; k++)
            if (!std::isfinite(sc->vertices[3 * (size_t)v + k])) {
                g_create_error = "vertex " + std::to_string(v) + " has a non-finite coordinate (" + "xyz"[k] + ")";
                return SPCBPT_ERR_INVALID_ARG;
            }
    for (int i = 0; i < sc->n_lights; i++)
        for (int k = 0; k < 3; k++) {
            const spcbpt_quad_light& s = sc->lights[i];
            const float corner_u = s.position[k] + s.u[k], corner_v = s.position[k] + s.v[k];   // the corners the emitter triangles get below
            if (!std::isfinite(s.position[k]) || !std::isfinite(s.u[k]) || !std::isfinite(s.v[k]) || !std::isfinite(corner_u) || !std::isfinite(corner_v) ||
                !std::isfinite(corner_u + corner_v - s.position[k])) {
                g_create_error = "quad light " + std::to_string(i) + " has a non-finite corner or edge (" + "xyz"[k] + ")";
                return SPCBPT_ERR_INVALID_ARG;
            }
        }
    for (int t = 0; t < sc->n_triangles; t++) {
        for (int k = 0; k < 3; k++)
            if (sc->indices[3 * (size_t)t + k] >= (uint32_t)sc->n_vertices) {
                g_create_error = "vertex index out of range (triangle " + std::to_string(t) + ": index " + std::to_string(sc->indices[3 * (size_t)t + k]) + " of " + std::to_string(sc->n_vertices) + " vertices)";
                return SPCBPT_ERR_INVALID_ARG;
            }
        if (sc->tri_material[t] < 0 || sc->tri_material[t] >= sc->n_materials) { g_create_error = "material index out of range"; return SPCBPT_ERR_INVALID_ARG; }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_create_error = "no HIP device available (the MI355X path has no CPU fallback)"; return SPCBPT_ERR_NO_DEVICE; }
    if (device < 0 || device >= ndev) { g_create_error = "device ordinal out of range"; return SPCBPT_ERR_NO_DEVICE; }
    if (hipSetDevice(device) != hipSuccess) { g_create_error = "hipSetDevice failed"; return SPCBPT_ERR_NO_DEVICE; }
    int patches = 0;
    for (int i = 0; i < sc->n_lights; i++) {
        if (sc->lights[i].div_level < 1) { g_create_error = "light div_level must be >= 1"; return SPCBPT_ERR_INVALID_ARG; }
        patches += sc->lights[i].div_level * sc->lights[i].div_level;
    }
    if (patches > SPCBPT_NUM_SUBSPACE_LIGHTSOURCE) { g_create_error = "sum of div_level^2 exceeds NUM_SUBSPACE_LIGHTSOURCE (200)"; return SPCBPT_ERR_INVALID_ARG; }
    if (sc->n_materials + sc->n_lights > 32767) { g_create_error = "too many materials (int16 material ids)"; return SPCBPT_ERR_INVALID_ARG; }
    // mesh lights: every named material once, in range, on at least one triangle with area; their patches share the quads' budget
    std::vector<MeshLightTable> ml_tables((size_t)std::max(n_ml, 0));
    std::vector<std::vector<int32_t>> ml_tris((size_t)std::max(n_ml, 0));   // scene triangles of the light's material
    for (int j = 0; j < n_ml; j++) {
        const spcbpt_mesh_light& m = ml[j];
        const std::string who = "mesh light " + std::to_string(j);
        if (m.material < 0 || m.material >= sc->n_materials) { g_create_error = who + ": material index out of range"; return SPCBPT_ERR_INVALID_ARG; }
        for (int k = 0; k < j; k++) if (ml[k].material == m.material) { g_create_error = who + ": material " + std::to_string(m.material) + " is named twice"; return SPCBPT_ERR_INVALID_ARG; }
        if (m.n_patches < 1) { g_create_error = who + ": n_patches must be >= 1"; return SPCBPT_ERR_INVALID_ARG; }
        for (int k = 0; k < 3; k++) if (!(m.emission[k] >= 0.0f) || !std::isfinite(m.emission[k])) { g_create_error = who + ": emission must be finite and >= 0"; return SPCBPT_ERR_INVALID_ARG; }
        patches += m.n_patches;
        if (patches > SPCBPT_NUM_SUBSPACE_LIGHTSOURCE) { g_create_error = "sum of div_level^2 and mesh-light n_patches exceeds NUM_SUBSPACE_LIGHTSOURCE (200)"; return SPCBPT_ERR_INVALID_ARG; }
        std::vector<uint32_t> idx;
        for (int t = 0; t < sc->n_triangles; t++)
            if (sc->tri_material[t] == m.material) { ml_tris[(size_t)j].push_back(t); idx.insert(idx.end(), sc->indices + 3 * (size_t)t, sc->indices + 3 * (size_t)t + 3); }
        if (ml_tris[(size_t)j].empty()) { g_create_error = who + ": material " + std::to_string(m.material) + " is used by no triangle"; return SPCBPT_ERR_INVALID_ARG; }
        build_mesh_light_table(sc->vertices, idx.data(), (int)ml_tris[(size_t)j].size(), m.n_patches, ml_tables[(size_t)j]);
        if (ml_tables[(size_t)j].tri.empty() || !((float)ml_tables[(size_t)j].area > 0.0f)) { g_create_error = "degenerate mesh light (" + who + ": no triangle with area)"; return SPCBPT_ERR_INVALID_ARG; }
    }
    if (sc->n_materials + sc->n_lights + n_ml > 32767) { g_create_error = "too many materials (int16 material ids)"; return SPCBPT_ERR_INVALID_ARG; }

    spcbpt_ctx* c = new spcbpt_ctx();
    c->device = device;
#define CREATE_TRY(expr)                                                                                           \
    do {                                                                                                           \
        hipError_t e__ = (expr);                                                                                   \
        if (e__ != hipSuccess) { g_create_error = std::string(#expr) + ": " + hipGetErrorString(e__); delete c; return SPCBPT_ERR_HIP; } \
    } while (0)
    // non-blocking streams: a host that drives collectives on the legacy default stream (torch) must not be serialised with
    // the render stream; every hand-over in this file is an explicit event or synchronize
    // Priorities: the light pass, the sampler build and the exchange copies are small, latency-critical kernels that the host
    // (or the next eye launch) waits for, while several persistent eye kernels queue for every block slot that frees up; the
    // light stream therefore gets the highest priority and the render streams the lowest (SPCBPT_STREAM_PRIORITY=0: all equal).
    int prio_least = 0, prio_greatest = 0;
    CREATE_TRY(hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    const char* sp = getenv("SPCBPT_STREAM_PRIORITY");
    const bool use_prio = !(sp && std::string(sp) == "0") && prio_least != prio_greatest;
    if (use_prio) CREATE_TRY(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_greatest));
    else CREATE_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    {
        const char* ov = getenv("SPCBPT_OVERLAP");
        const char* nr = getenv("SPCBPT_RENDER_STREAMS");
        c->n_render = nr ? std::max(1, std::min((int)Context::kMaxRender, atoi(nr))) : 2;
        if (ov && std::string(ov) == "0") c->n_render = 1;
        if (const char* eb = getenv("SPCBPT_EYE_BATCH")) c->eye_batch = std::max(1, std::min((int)kMaxBatchFrames, atoi(eb)));
        // sets: one per frame of every eye launch in flight + the light passes ahead of them + the one being built
        c->n_sets = std::min((int)Context::kMaxSets, c->eye_batch > 1 ? c->eye_batch * (c->n_render + 2) + 3 : c->n_render + 4);   // batches in flight + one being built + a batch of light passes ahead
        if (const char* sb = getenv("SPCBPT_SAMPLER_BUILD")) c->counting_build = std::string(sb) != "hipcub";
        if (const char* lc = getenv("SPCBPT_LVC_CAPACITY")) c->lvc_fixed = (size_t)std::max(0ll, atoll(lc));   // vertices per buffer set (0 = probe)
        if (const char* ns = getenv("SPCBPT_SETS")) c->n_sets = std::max(3, std::min((int)Context::kMaxSets, atoi(ns)));   // developer knob
        for (int s = 0; s < c->n_render; s++) {
            if (ov && std::string(ov) == "0") c->rstreams[s] = c->stream;
            else if (use_prio) CREATE_TRY(hipStreamCreateWithPriority(&c->rstreams[s], hipStreamNonBlocking, prio_least));
            else CREATE_TRY(hipStreamCreateWithFlags(&c->rstreams[s], hipStreamNonBlocking));
            CREATE_TRY(hipEventCreateWithFlags(&c->ev_merge[s].ev, hipEventDisableTiming));
        }
        c->rstream = c->rstreams[0];
        c->lanes[0].stream = c->stream;
        for (int s = 0; s < c->n_sets; s++) {
            CacheSet& S = c->sets[s];
            for (Event* e : {&S.sampler, &S.render, &S.light, &S.on_stream, &S.exch}) CREATE_TRY(hipEventCreateWithFlags(&e->ev, hipEventDisableTiming));
        }
        CREATE_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->h_import_counts), (size_t)Context::kMaxSets * 2 * sizeof(int)));
        CREATE_TRY(hipHostMalloc(reinterpret_cast<void**>(&c->h_light_counts), (size_t)Context::kMaxSets * 2 * sizeof(int)));
    }

    // ---- scene assembly (scene_shift.cpp:64-154, 184-328)
    std::vector<float> V(sc->vertices, sc->vertices + 3 * (size_t)sc->n_vertices);
    std::vector<float> UV(2 * (size_t)sc->n_vertices, 0.0f);
    if (sc->texcoords) UV.assign(sc->texcoords, sc->texcoords + 2 * (size_t)sc->n_vertices);
    std::vector<uint32_t> I(sc->indices, sc->indices + 3 * (size_t)sc->n_triangles);
    std::vector<int32_t> TM(sc->tri_material, sc->tri_material + sc->n_triangles);
    std::vector<uint8_t> EM(sc->n_triangles, 0);
    std::vector<DMaterial> mats;
    for (int i = 0; i < sc->n_materials; i++) {
        const spcbpt_material& m = sc->materials[i];
        if (m.albedo_tex < 0 || m.albedo_tex > sc->n_textures) { g_create_error = "albedo_tex out of range"; delete c; return SPCBPT_ERR_INVALID_ARG; }
        DMaterial d;
        memset(&d, 0, sizeof(d));
        memcpy(d.base_color, m.base_color, 12);
        d.metallic = m.metallic; d.roughness = m.roughness; d.specular = m.specular; d.specular_tint = m.specular_tint;
        d.subsurface = m.subsurface; d.sheen = m.sheen; d.sheen_tint = m.sheen_tint; d.clearcoat = m.clearcoat;
        d.clearcoat_gloss = m.clearcoat_gloss; d.albedo_tex = m.albedo_tex; d.light_id = -1;
        d.brdf = m.brdf != 0;   // Pbr::brdf is a bool (MaterialData.h:99) assigned from the scene file's int (scene_shift.cpp:75)
        mats.push_back(d);
    }
    std::vector<DLight> lights;
    int ss_base = 0;
    for (int i = 0; i < sc->n_lights; i++) {
        const spcbpt_quad_light& s = sc->lights[i];
        DLight L;
        memset(&L, 0, sizeof(L));
        float cr[3] = {s.u[1] * s.v[2] - s.u[2] * s.v[1], s.u[2] * s.v[0] - s.u[0] * s.v[2], s.u[0] * s.v[1] - s.u[1] * s.v[0]};
        float len = sqrtf(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
        if (!(len > 0)) { g_create_error = "degenerate quad light"; delete c; return SPCBPT_ERR_INVALID_ARG; }
        float inv = 1.0f / len;
        for (int k = 0; k < 3; k++) {
            L.corner[k] = s.position[k]; L.u[k] = s.position[k] + s.u[k]; L.v[k] = s.position[k] + s.v[k];
            L.emission[k] = s.emission[k]; L.normal[k] = cr[k] * inv;
        }
        L.area = len; L.div_level = s.div_level; L.ss_base = ss_base; L.id = (int)lights.size();
        ss_base += s.div_level * s.div_level;
        lights.push_back(L);
        DMaterial d;  // emissive pseudo-material with MaterialData() defaults
        memset(&d, 0, sizeof(d));
        d.base_color[0] = d.base_color[1] = d.base_color[2] = 1.0f; d.metallic = 1.0f; d.roughness = 1.0f; d.specular = 0.5f;
        d.sheen_tint = 0.5f; d.clearcoat_gloss = 1.0f; d.light_id = i;
        mats.push_back(d);
        uint32_t base = (uint32_t)(V.size() / 3);
        float p3[3] = {L.u[0] + L.v[0] - L.corner[0], L.u[1] + L.v[1] - L.corner[1], L.u[2] + L.v[2] - L.corner[2]};
        V.insert(V.end(), L.corner, L.corner + 3); V.insert(V.end(), L.u, L.u + 3); V.insert(V.end(), L.v, L.v + 3); V.insert(V.end(), p3, p3 + 3);
        const float quv[8] = {0, 0, 1, 0, 0, 1, 1, 1};
        UV.insert(UV.end(), quv, quv + 8);
        const uint32_t qi[6] = {base, base + 1, base + 3, base, base + 3, base + 2};
        I.insert(I.end(), qi, qi + 6);
        TM.push_back((int)mats.size() - 1); TM.push_back((int)mats.size() - 1);
        EM.push_back(1); EM.push_back(1);
        c->h_light_tris.push_back(2);
    }
    // Mesh lights (completing sutil/Scene.cpp:1739-1743, which routes emissive meshes to the emitter programs, with the sampler
    // cuProg.h:554-666 lacks): the light's triangles get its pseudo-material and corners of their own whose UVs carry the patch
    // (patch + 0.5 at all three corners, so that the interpolated u floors to the patch whatever the barycentrics round to) --
    // the label of a hit needs no table, the triangle record stays 64 B.
    for (int j = 0; j < n_ml; j++) {
        const MeshLightTable& T = ml_tables[(size_t)j];
        const int n = (int)T.tri.size();
        DLight L;
        memset(&L, 0, sizeof(L));
        L.area = (float)T.area; L.div_level = T.n_patches; L.ss_base = ss_base; L.id = (int)lights.size(); L.type = 2;
        for (int k = 0; k < 3; k++) L.emission[k] = ml[j].emission[k];
        ss_base += T.n_patches;
        DMaterial d;
        memset(&d, 0, sizeof(d));
        d.base_color[0] = d.base_color[1] = d.base_color[2] = 1.0f; d.metallic = 1.0f; d.roughness = 1.0f; d.specular = 0.5f;
        d.sheen_tint = 0.5f; d.clearcoat_gloss = 1.0f; d.light_id = L.id;
        mats.push_back(d);
        const int padded = (n + 7) / 8 * 8 + 8, buckets = mesh_light_guide_buckets(n);
        std::vector<uint32_t> guide;
        build_mesh_light_guide(T.cmf, buckets, guide);
        const size_t rec_off = c->h_etable.size() / 4, cmf_off = rec_off + (size_t)MESH_LIGHT_REC_QUADS * n, guide_off = cmf_off + (size_t)padded / 4;
        c->h_etable.resize((guide_off + (size_t)buckets / 4) * 4, 0.0f);
        const int32_t words[6] = {(int32_t)rec_off, (int32_t)cmf_off, (int32_t)guide_off, n, buckets, padded};
        memcpy(L.corner, words, 12); memcpy(L.u, words + 3, 12);
        for (int i = 0; i < n; i++) {
            const int t = ml_tris[(size_t)j][(size_t)T.tri[(size_t)i]];
            const uint32_t base = (uint32_t)(V.size() / 3);
            float P[3][3];
            for (int v = 0; v < 3; v++) {
                memcpy(P[v], sc->vertices + 3 * (size_t)sc->indices[3 * (size_t)t + v], 12);
                V.insert(V.end(), P[v], P[v] + 3);
                UV.push_back((float)T.patch[(size_t)i] + 0.5f); UV.push_back(0.0f);
                I[3 * (size_t)t + v] = base + (uint32_t)v;
            }
            TM[(size_t)t] = (int)mats.size() - 1;
            EM[(size_t)t] = 1;
            float* r = &c->h_etable[(rec_off + (size_t)MESH_LIGHT_REC_QUADS * i) * 4];
            for (int k = 0; k < 3; k++) { r[k] = P[0][k]; r[4 + k] = P[1][k] - P[0][k]; r[8 + k] = P[2][k] - P[0][k]; }
            r[3] = T.cmf[(size_t)i];
            memcpy(r + 7, &T.patch[(size_t)i], 4);
        }
        float* cm = &c->h_etable[cmf_off * 4];
        for (int i = 0; i < padded; i++) cm[i] = i < n ? T.cmf[(size_t)i] : 2.0f;
        memcpy(&c->h_etable[guide_off * 4], guide.data(), (size_t)buckets * 4);
        lights.push_back(L);
        c->h_light_tris.push_back(n);
    }
    HostMesh mesh;
    mesh.vertices = V.data(); mesh.texcoords = UV.data(); mesh.indices = I.data(); mesh.tri_material = TM.data(); mesh.tri_emitter = EM.data();
    mesh.n_vertices = (int)(V.size() / 3); mesh.n_triangles = (int)(I.size() / 3);
    Lbvh bvh;
    build_lbvh(mesh, bvh);
    c->n_triangles = mesh.n_triangles; c->n_nodes = (int)(bvh.nodes.size() / 16); c->bvh_depth = bvh.depth;
    c->n_lights = (int)lights.size(); c->n_mats = (int)mats.size();

    // nodes and the PAIR records of the triangles (lbvh.h: Lbvh::pairs, one 64-B slot per triangle) in ONE allocation, the pair records
    // right behind the node records: the pooled traversal step fetches "the record of its next step" through one base pointer
    // (dev_traversal.h: SPC_FETCH_STEP__).  The per-triangle records (corners + UVs + material: what the tails, the one-ray-per-lane
    // loop and the shading read) live in an allocation of their own.
    CREATE_TRY(c->d_nodes.reserve(bvh.nodes.size() + bvh.pairs.size()));
    CREATE_TRY(c->d_tris.reserve(bvh.tris.size()));
    if (getenv("SPCBPT_NO_TRI_PAIRS")) {   // test switch: every slot a single triangle (the same device code, one test per step): films must not change
        for (size_t i = 0; i < bvh.pairs.size() / 16; i++) { uint32_t fl; memcpy(&fl, &bvh.pairs[i * 16 + 15], 4); fl &= 0x80000000u; memcpy(&bvh.pairs[i * 16 + 15], &fl, 4); }
        bvh.n_paired = 0;
    }
    CREATE_TRY(hipMemcpy(c->d_nodes + bvh.nodes.size(), bvh.pairs.data(), bvh.pairs.size() * 4, hipMemcpyHostToDevice));
    c->n_paired = bvh.n_paired;
    CREATE_TRY(c->d_tri_orig.reserve(bvh.tri_orig.size()));
    CREATE_TRY(c->d_mats.reserve(mats.size()));
    CREATE_TRY(hipMemcpy(c->d_nodes, bvh.nodes.data(), bvh.nodes.size() * 4, hipMemcpyHostToDevice));
    CREATE_TRY(hipMemcpy(c->d_tris, bvh.tris.data(), bvh.tris.size() * 4, hipMemcpyHostToDevice));
    CREATE_TRY(hipMemcpy(c->d_tri_orig, bvh.tri_orig.data(), bvh.tri_orig.size() * 4, hipMemcpyHostToDevice));
    CREATE_TRY(hipMemcpy(c->d_mats, mats.data(), mats.size() * sizeof(DMaterial), hipMemcpyHostToDevice));
    c->h_lights = lights;
    for (int k = 0; k < 3; k++) { c->bbox_lo[k] = 1e30f; c->bbox_hi[k] = -1e30f; }
    for (size_t i = 0; i < V.size(); i += 3)
        for (int k = 0; k < 3; k++) { c->bbox_lo[k] = std::min(c->bbox_lo[k], V[i + k]); c->bbox_hi[k] = std::max(c->bbox_hi[k], V[i + k]); }
    std::vector<DTexture> texs;
    for (int i = 0; i < sc->n_textures; i++) {
        const spcbpt_texture& t = sc->textures[i];
        if (!t.rgba || t.width < 1 || t.height < 1) { g_create_error = "bad texture"; delete c; return SPCBPT_ERR_INVALID_ARG; }
        uint32_t* d = nullptr;
        CREATE_TRY(dev_alloc(&d, (size_t)t.width * t.height));
        c->d_tex_data.push_back(d);
        CREATE_TRY(hipMemcpy(d, t.rgba, (size_t)t.width * t.height * 4, hipMemcpyHostToDevice));
        texs.push_back(DTexture{d, t.width, t.height});
    }
    CREATE_TRY(c->d_tex.reserve(texs.size()));
    if (!texs.empty()) CREATE_TRY(hipMemcpy(c->d_tex, texs.data(), texs.size() * sizeof(DTexture), hipMemcpyHostToDevice));
    CREATE_TRY(c->d_set_counts_all.reserve((size_t)2 * Context::kMaxSets + 2));   // + a spare pair (probe_lvc_capacity)
    CREATE_TRY(hipMemset(c->d_set_counts_all, 0, (2 * Context::kMaxSets + 2) * sizeof(int)));
    for (int s = 0; s < c->n_sets; s++) {
        CREATE_TRY(c->sets[s].subspace.reserve((size_t)SPCBPT_NUM_SUBSPACE));
        c->sets[s].counts = c->d_set_counts_all + 2 * s;
    }
    {
        hipDeviceProp_t prop;
        CREATE_TRY(hipGetDeviceProperties(&prop, device));
        c->num_cus = prop.multiProcessorCount;
    }
    CREATE_TRY(c->d_work_counter.reserve((size_t)Context::kMaxRender + 2));   // tile queues of the render streams + core queues of the two light lanes
    for (int lane = 0; lane < 2; lane++) c->lanes[lane].work_counter = c->d_work_counter + Context::kMaxRender + lane;
    CREATE_TRY(c->d_diag.reserve((size_t)4));
    CREATE_TRY(hipMemset(c->d_diag, 0, 4 * sizeof(uint32_t)));
    if (const char* e = getenv("SPCBPT_DEBUG_SPILL_ENTRIES")) c->spill_entries_debug = std::max(0, atoi(e));
    CREATE_TRY(c->d_counters.reserve((size_t)C_COUNT));
    CREATE_TRY(hipMemset(c->d_counters, 0, C_COUNT * sizeof(unsigned long long)));
    memset(&c->kp, 0, sizeof(c->kp));
    if (c->upload_lights()) { g_create_error = c->error; delete c; return SPCBPT_ERR_HIP; }
    c->kp.scene.nodes = c->d_nodes; c->kp.scene.tris = c->d_tris; c->kp.scene.tri_base = c->n_nodes; c->kp.scene.tri_orig = c->d_tri_orig; c->kp.scene.mats = c->d_mats;
    c->kp.scene.lights = c->d_lights; c->kp.scene.tex = c->d_tex; c->kp.scene.n_lights = c->n_lights; c->kp.scene.n_mats = c->n_mats;
    // the same nodes, one record per child: the quad tail of the pooled traversal pass (device_lib.h) and the traversal A/B harness
    CREATE_TRY(c->d_nodes_q.reserve((size_t)c->n_nodes * 16));
    launch_repack_nodes_quad(c->d_nodes, c->d_nodes_q, c->n_nodes, c->stream);
    CREATE_TRY(hipGetLastError());
    CREATE_TRY(hipStreamSynchronize(c->stream));
    c->kp.scene.nodes_q = getenv("SPCBPT_NO_QUAD_TAIL") ? nullptr : c->d_nodes_q.p;
    c->kp.scene.fan_tail = getenv("SPCBPT_NO_FAN_TAIL") ? 0 : 1;
    c->kp.scene.general = 0;   // no environment map yet; a flagged material (Pbr::brdf) selects the general kernels as well
    for (const DMaterial& m : mats) if (m.brdf) c->kp.scene.general = 1;
    if (n_ml > 0) c->kp.scene.general = 1;   // the mesh branch of eye_emitter_hit lives in the general forms only (eye_walk.h)
    c->kp.sampler_counts = c->sets[0].counts;
    c->kp.diag = c->d_diag;
    c->kp.row_step = 1;
    CREATE_TRY(hipDeviceSynchronize());   // the uploads above went through the default stream; the context's streams do not wait for it
#undef CREATE_TRY
    *out = c;
    return SPCBPT_OK;
}

extern "C" {

int spcbpt_create(const spcbpt_scene_desc* sc, int device, spcbpt_ctx** out) { return create_context(sc, nullptr, 0, device, out); }

int spcbpt_create_lit(const spcbpt_scene_desc* sc, const spcbpt_mesh_light* mesh_lights, int n_mesh_lights, int device, spcbpt_ctx** out) {
    if (n_mesh_lights < 0 || (n_mesh_lights > 0 && !mesh_lights)) { g_create_error = "create_lit: null mesh-light array"; if (out) *out = nullptr; return SPCBPT_ERR_INVALID_ARG; }
    static const spcbpt_mesh_light none = {0, {0, 0, 0}, 1};
    return create_context(sc, n_mesh_lights > 0 ? mesh_lights : &none, n_mesh_lights, device, out);
}
int spcbpt_mesh_light_struct_size(void) { return (int)sizeof(spcbpt_mesh_light); }

int spcbpt_light_info(spcbpt_ctx* c, int light, int32_t* type, float* area, int32_t* n_triangles, int32_t* first_subspace, int32_t* n_patches) {
    CTX_CHECK(c);
    if (light < 0 || light >= (int)c->h_lights.size()) { c->error = "light_info: light index out of range (" + std::to_string(c->h_lights.size()) + " lights)"; return SPCBPT_ERR_INVALID_ARG; }
    const DLight& L = c->h_lights[(size_t)light];
    const DEnv& E = c->kp.scene.env;
    if (type) *type = L.type;
    if (area) *area = L.type == 1 ? 0.0f : L.area;
    if (n_triangles) *n_triangles = light < (int)c->h_light_tris.size() ? c->h_light_tris[(size_t)light] : 0;
    if (first_subspace) *first_subspace = SPCBPT_NUM_SUBSPACE - 1 - (L.type == 1 ? 0 : L.ss_base);
    if (n_patches) *n_patches = L.type == 1 ? E.div_level * E.div_level : (L.type == 2 ? L.div_level : L.div_level * L.div_level);
    return SPCBPT_OK;
}

int spcbpt_destroy(spcbpt_ctx* c) {
    if (!c) return SPCBPT_ERR_INVALID_ARG;
    spc_viewers_forget_context(c);   // viewers of this context live on as state machines without one (viewer.cpp)
    (void)hipSetDevice(c->device);
    (void)c->sync_all();
    delete c;
    return SPCBPT_OK;
}

const char* spcbpt_build_arithmetic(void) {
#if defined(SPCBPT_FAST_MATH_BUILD)
    return "approx";
#else
    return "ieee";
#endif
}

const char* spcbpt_last_error(const spcbpt_ctx* c) { return c ? c->error.c_str() : g_create_error.c_str(); }


int spcbpt_set_camera(spcbpt_ctx* c, const float eye[3], const float U[3], const float V[3], const float W[3]) {
    CTX_CHECK(c);
    if (!eye || !U || !V || !W) { c->error = "null camera vector"; return SPCBPT_ERR_INVALID_ARG; }
    memcpy(c->kp.eye, eye, 12); memcpy(c->kp.U, U, 12); memcpy(c->kp.V, V, 12); memcpy(c->kp.W, W, 12);
    c->have_camera = true;
    c->update_lens_axes();   // (ctx_lens.hip: the lens stays, its axes follow the frame)
    return SPCBPT_OK;
}

int spcbpt_set_camera_lookat(spcbpt_ctx* c, const float eye[3], const float lookat[3], const float up[3], float fov, float aspect) {
    CTX_CHECK(c);
    if (!eye || !lookat || !up) { c->error = "null camera vector"; return SPCBPT_ERR_INVALID_ARG; }
    // sutil::Camera::UVWFrame (sutil/Camera.cpp:34-45)
    auto cross = [](const float* a, const float* b, float* r) { r[0] = a[1] * b[2] - a[2] * b[1]; r[1] = a[2] * b[0] - a[0] * b[2]; r[2] = a[0] * b[1] - a[1] * b[0]; };
    auto norm = [](float* v) { float inv = 1.0f / sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); v[0] *= inv; v[1] *= inv; v[2] *= inv; };
    float W[3] = {lookat[0] - eye[0], lookat[1] - eye[1], lookat[2] - eye[2]}, U[3], V[3];
    float wlen = sqrtf(W[0] * W[0] + W[1] * W[1] + W[2] * W[2]);
    cross(W, up, U); norm(U);
    cross(U, W, V); norm(V);
    float vlen = wlen * tanf(0.5f * fov * 3.14159265358979323846f / 180.0f);
    for (int k = 0; k < 3; k++) V[k] *= vlen;
    float ulen = vlen * aspect;
    for (int k = 0; k < 3; k++) U[k] *= ulen;
    return spcbpt_set_camera(c, eye, U, V, W);
}

int spcbpt_resize(spcbpt_ctx* c, int w, int h) {
    CTX_CHECK(c);
    if (w < 1 || h < 1 || (long long)w * h > (1ll << 28)) { c->error = "bad image size"; return SPCBPT_ERR_INVALID_ARG; }
    if (c->sync_all()) return SPCBPT_ERR_HIP;
    c->deferred.active = false;   // a deferred frame of the old size is dropped with its buffer
    c->adaptive_drop();           // adaptive sampling ends with the film its tiles belong to
    c->d_accum.release(); c->d_frame.release();
    c->free_features();           // feature buffers and denoiser planes of the old size: re-allocated on demand
    c->free_guides();             // ... and the reflected guide planes
    c->free_moments();            // ... and the film's second moment
    c->free_buckets();            // ... and the bucket film with its resolved image (K stays)
    c->free_display();            // ... and the display plane with its record: the previous EV is forgotten
    c->free_bloom();              // ... and the bloom plane with its pyramid
    c->free_local_tone();         // ... and the local tone plane with its grid buffers
    c->free_history();            // ... and the history, its prior and the resolved image
    c->splat_records_rk = -1;     // the records of an ordered "lt" launch belong to the old film (their buffers follow the cache capacity and stay)
    HIP_TRY(c, c->d_accum.reserve((size_t)w * h * 4));
    HIP_TRY(c, c->d_frame.reserve((size_t)w * h));
    for (auto& slots : c->d_result_b) for (auto& r : slots) r.release();   // re-allocated at the new size on demand
    for (int s = 0; s < c->n_render; s++) {
        c->d_result[s].release();
        HIP_TRY(c, c->d_result[s].reserve((size_t)w * h * 4));
    }
    HIP_TRY(c, hipMemsetAsync(c->d_accum, 0, (size_t)w * h * 16, c->rstream));
    HIP_TRY(c, hipMemsetAsync(c->d_frame, 0, (size_t)w * h * 4, c->rstream));
    HIP_TRY(c, hipStreamSynchronize(c->rstream));
    c->kp.width = w; c->kp.height = h; c->kp.accum = c->d_accum; c->kp.frame = c->d_frame;
    return SPCBPT_OK;
}

int spcbpt_set_subspace(spcbpt_ctx* c, const spcbpt_tree_node* et, int ne, const spcbpt_tree_node* lt, int nl, const float* q, const float* g) {
    CTX_CHECK(c);
    if (!et && !lt && !q && !g) return c->install_minimal_tuple();
    return c->install_subspace(et, ne, lt, nl, q, g);
}

int spcbpt_set_environment(spcbpt_ctx* c, const float* rgba, int width, int height, const float* center, float radius) {
    CTX_CHECK(c);
    return c->set_environment(rgba, width, height, center, radius);
}
int spcbpt_get_environment(spcbpt_ctx* c, int* width, int* height, float center[3], float* radius, int* n_lights) {
    CTX_CHECK(c);
    const DEnv& V = c->kp.scene.env;
    if (width) *width = V.valid ? V.width : 0;
    if (height) *height = V.valid ? V.height : 0;
    if (center) memcpy(center, V.center, 12);
    if (radius) *radius = V.valid ? V.r : 0.0f;
    if (n_lights) *n_lights = c->n_lights;
    return SPCBPT_OK;
}
int spcbpt_set_environment_mode(spcbpt_ctx* c, int flags) {
    CTX_CHECK(c);
    if (flags & ~(SPCBPT_ENV_EYE_SEES_SKY | SPCBPT_ENV_PT_SKY_SHADOW_ALONG_DIR)) { c->error = "set_environment_mode: unknown flag bits"; return SPCBPT_ERR_INVALID_ARG; }
    if (c->deferred.active) { c->error = "set_environment_mode: a deferred frame is outstanding: spcbpt_merge_deferred(ctx, keep) first"; return SPCBPT_ERR_STATE; }
    if (c->sync_all()) return SPCBPT_ERR_HIP;
    c->kp.scene.env.mode = flags;
    c->blocks_per_cu[0] = c->blocks_per_cu_batch = c->blocks_per_cu_lens = 0;   // the timed eye launches may change instantiation: ask again
    return SPCBPT_OK;
}
int spcbpt_get_environment_mode(spcbpt_ctx* c, int* flags) {
    CTX_CHECK(c);
    if (!flags) return SPCBPT_ERR_INVALID_ARG;
    *flags = c->kp.scene.env.mode;
    return SPCBPT_OK;
}

int spcbpt_set_light_trace(spcbpt_ctx* c, const spcbpt_light_trace_params* p) {
    CTX_CHECK(c);
    if (!p) { c->error = "null params"; return SPCBPT_ERR_INVALID_ARG; }
    if (c->sync_all()) return SPCBPT_ERR_HIP;
    return c->set_light_trace(*p);
}

int spcbpt_lvc_set_capacity(spcbpt_ctx* c, int vertices) {
    CTX_CHECK(c);
    if (vertices < 0) { c->error = "lvc_set_capacity: negative capacity"; return SPCBPT_ERR_INVALID_ARG; }
    c->lvc_fixed = (size_t)vertices;
    if (c->sbb_keys) { if (c->sync_all()) return SPCBPT_ERR_HIP; c->free_batch_build_scratch(); }   // sized for the old capacity's builds
    c->sbb_refused_bytes = 0;
    if (vertices == 0) { c->lvc_probe_needed = true; return SPCBPT_OK; }   // back to the probe pass (the sets only ever grow)
    c->lvc_probe_needed = false;
    return c->ensure_lvc_capacity((size_t)vertices);
}
int spcbpt_lvc_get_capacity(spcbpt_ctx* c, int* vertices, int* sets) {
    CTX_CHECK(c);
    if (vertices) *vertices = (int)std::min<size_t>(c->lvc_capacity, 0x7fffffff);
    if (sets) *sets = c->n_sets;
    return SPCBPT_OK;
}

int spcbpt_launch(spcbpt_ctx* c, const char* name, uint32_t frame, int r0, int r1, int rs) {
    CTX_CHECK(c);
    if (!name) { c->error = "null algorithm name"; return SPCBPT_ERR_INVALID_ARG; }
    const std::string alg(name);
    if (alg == "light trace") return c->launch_light(frame);
    if (alg == "SPCBPT_eye") return c->launch_render("spcbpt_render", true, frame, r0, r1, rs);
    if (alg == "pt") return c->launch_render("pt", false, frame, r0, r1, rs);
    if (alg == "SPCBPT_no_rmis") return c->launch_render("spcbpt_no_rmis", true, frame, r0, r1, rs, true);   // raygen.cu:465: defined upstream, wired to no program group
    if (alg == "pretrace") return c->launch_pretrace(frame);
    if (alg == "lt") return c->launch_splat(frame, r0, r1, rs);   // light tracing: the cache splatted onto the film (ctx_splat.hip)
    c->error = "unknown algorithm '" + alg + "' (expected \"pt\", \"light trace\", \"SPCBPT_eye\", \"pretrace\", \"SPCBPT_no_rmis\" or \"lt\")";
    return SPCBPT_ERR_UNKNOWN_ALG;
}

int spcbpt_launch_deferred(spcbpt_ctx* c, const char* name, uint32_t frame, int r0, int r1, int rs) {
    CTX_CHECK(c);
    if (!name) { c->error = "null algorithm name"; return SPCBPT_ERR_INVALID_ARG; }
    const std::string alg(name);
    if (alg == "SPCBPT_eye") return c->launch_render("spcbpt_render", true, frame, r0, r1, rs, false, true);
    if (alg == "pt") return c->launch_render("pt", false, frame, r0, r1, rs, false, true);
    c->error = "launch_deferred: \"pt\" or \"SPCBPT_eye\"";
    return SPCBPT_ERR_UNKNOWN_ALG;
}
int spcbpt_merge_deferred(spcbpt_ctx* c, int keep) { CTX_CHECK(c); return c->merge_deferred(keep != 0); }
int spcbpt_sync_film(spcbpt_ctx* c) { CTX_CHECK(c); return c->sync_film(); }

int spcbpt_launch_eye_batch(spcbpt_ctx* c, int n_frames, const uint32_t* subframes, int r0, int r1, int rs) {
    CTX_CHECK(c);
    return c->launch_eye_batch(n_frames, subframes, r0, r1, rs);
}
int spcbpt_launch_eye_batch_film(spcbpt_ctx* c, int n_frames, const uint32_t* subframes, int r0, int r1, int rs) {
    CTX_CHECK(c);
    return c->launch_eye_batch_film(n_frames, subframes, r0, r1, rs);
}

int spcbpt_build_sampler_batch(spcbpt_ctx* c, int n_builds) {
    CTX_CHECK(c);
    return c->build_sampler_batch(n_builds);
}
int spcbpt_launch_light_batch(spcbpt_ctx* c, uint32_t first_frame, int n_frames) {
    CTX_CHECK(c);
    return c->launch_light_batch(first_frame, n_frames);
}

int spcbpt_build_sampler(spcbpt_ctx* c) {
    CTX_CHECK(c);
    return c->build_sampler();
}

}  // extern "C"
