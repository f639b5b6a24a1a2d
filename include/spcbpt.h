/*
 * spcbpt.h — C ABI of the MI355X-native SPCBPT hot path.
 *
 * This is the drop-in boundary for the path BASELINE.json's north_star names:
 * light sub-path tracing -> light-vertex-cache (LVC) sampler build -> eye
 * sub-path tracing with subspace classification, two-stage resampling through
 * the subspace sampling matrix, shadow ray, BSDF + recursive-MIS connection,
 * accumulation.  Every entry point cites the reference interface it replaces
 * (paths relative to the reference checkout's src/ directory).
 *
 * The reference dispatches this path by *name* through
 *   sutil::Scene::switchRaygen("pt" | "light trace" | "SPCBPT_eye" | "pretrace")
 *   (sutil/Scene.cpp:1642-1789) followed by optixLaunch(pipeline, 0, d_params,
 *   sizeof(MyParams), sbt, w, h, 1) (OptiXPathTracer/optixPathTracer.cpp:503-512,
 *   535-544, 623-632).  spcbpt_launch() keeps the same four names.
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on
 * success or a negative spcbpt_status; nothing throws across the ABI; all
 * device memory is owned by the context; one context per GPU; calls on one
 * context are not re-entrant.  Launches are asynchronous on the context's HIP
 * stream; spcbpt_sync() waits.
 */
#ifndef SPCBPT_H
#define SPCBPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Compile-time constants of the reference (OptiXPathTracer/optixPathTracer.h:31-39). */
#define SPCBPT_NUM_SUBSPACE 1000             /* NUM_SUBSPACE */
#define SPCBPT_NUM_SUBSPACE_LIGHTSOURCE 200  /* NUM_SUBSPACE_LIGHTSOURCE = int(0.2*NUM_SUBSPACE) */
#define SPCBPT_CONNECTION_N 3                /* CONNECTION_N */
#define SPCBPT_MIN_RR_RATE 0.3f              /* MIN_RR_RATE */
#define SPCBPT_SCENE_EPSILON 1e-3f           /* cuProg.h:39 SCENE_EPSILON */

typedef enum spcbpt_status {
    SPCBPT_OK = 0,
    SPCBPT_ERR_INVALID_ARG = -1,
    SPCBPT_ERR_NO_DEVICE = -2,   /* no HIP device / HIP runtime failure at create */
    SPCBPT_ERR_HIP = -3,         /* a HIP call failed; see spcbpt_last_error */
    SPCBPT_ERR_UNKNOWN_ALG = -4, /* name is not one of the four launch names */
    SPCBPT_ERR_STATE = -5,       /* call order violated (e.g. SPCBPT_eye before a sampler exists) */
    SPCBPT_ERR_CAPACITY = -6,    /* a caller-provided buffer is too small */
    SPCBPT_ERR_IO = -7           /* a file could not be read / written or is malformed */
} spcbpt_status;

/* Disney-principled material; field set of MaterialData::Pbr
 * (cuda/MaterialData.h:82-100).  albedo_tex is 0 for "none", else texture
 * index + 1 (OptiXPathTracer/scene_shift.cpp:76-79 uses the same 1-based id).
 * brdf is MaterialData::Pbr::brdf (MaterialData.h:99; `brdf <int>` of a .scene
 * material block, sceneLoader.cpp:107 -> scene_shift.cpp:75): nonzero makes
 * the bidirectional programs divide the BSDF value by |N.L| at the five
 * un-guarded ternaries hit_program.cu:286, 384, raygen.cu:271, 278 and
 * rmis.h:105 (the `#ifdef BRDF` branches of Eval/Pdf are dead).  "pt"
 * (hit_program.cu:439-552) has no such division. */
typedef struct spcbpt_material {
    float base_color[3];
    float metallic;
    float roughness;
    float specular;
    float specular_tint;
    float subsurface;
    float sheen;
    float sheen_tint;
    float clearcoat;
    float clearcoat_gloss;
    int32_t albedo_tex;
    int32_t brdf;
} spcbpt_material;

/* 8-bit RGBA image, row 0 first, sampled bilinear + wrap, then pow(c, 2.2)
 * (scene_shift.cpp:40-61, hit_program.cu:182-198, cuProg.h:361-368). */
typedef struct spcbpt_texture {
    const uint8_t* rgba;
    int32_t width;
    int32_t height;
} spcbpt_texture;

/* Quad emitter as the `.scene` light{} block gives it
 * (sceneLoader.cpp:130-193): corner `position`, absolute corner points v1, v2
 * are stored as edges u = v1-position, v = v2-position.  div_level^2 emitter
 * patches become light subspaces allocated downward from id 999
 * (scene_shift.cpp:108-154, cuProg.h:586-589). */
typedef struct spcbpt_quad_light {
    float position[3];
    float u[3];
    float v[3];
    float emission[3];
    int32_t div_level;
} spcbpt_quad_light;

/* Flat triangle soup.  The library appends two triangles per quad light with
 * UVs (0,0)(1,0)(0,1)(1,1) and an emissive pseudo-material after the scene
 * materials, exactly as scene_shift.cpp:92-103, 252-328 does; those triangles
 * are single-sided for path rays and opaque to shadow rays. */
typedef struct spcbpt_scene_desc {
    const float* vertices;        /* 3 * n_vertices */
    const float* texcoords;       /* 2 * n_vertices, may be NULL (zeros, scene_shift.cpp:204-207) */
    int32_t n_vertices;
    const uint32_t* indices;      /* 3 * n_triangles */
    const int32_t* tri_material;  /* n_triangles, index into materials */
    int32_t n_triangles;
    const spcbpt_material* materials;
    int32_t n_materials;
    const spcbpt_texture* textures;
    int32_t n_textures;
    const spcbpt_quad_light* lights;
    int32_t n_lights;
} spcbpt_scene_desc;

/* Octree node of the subspace classifiers; values of classTree::tree_node
 * (decisionTree/classTree_common.h:11-38).  type: 0 position, 1 normal,
 * 2 direction.  leaf != 0 -> label is the subspace id. */
typedef struct spcbpt_tree_node {
    float mid[3];
    int32_t child[8];
    int32_t label;
    int32_t type;
    int32_t leaf;
} spcbpt_tree_node;

/* Launch geometry of the light pass = LightTraceParams
 * (optixPathTracer.h:52-66; reference values num_core 1000, core_padding 800,
 * M_per_core 100 from optixPathTracer.cpp:462-468).  Path index p of core c
 * draws its random numbers from the core's running seed tea<4>(c, frame).
 * The MI355X default is one light path per lane: num_core = M, M_per_core = 1. */
typedef struct spcbpt_light_trace_params {
    int32_t num_core;
    int32_t core_padding;
    int32_t m_per_core;
    int32_t core_begin; /* first core traced by this context (multi-GPU sharding) */
    int32_t core_count; /* number of cores traced by this context; 0 = all */
    /* 0 = reference behaviour: the BSDF stream (payload.seed) starts equal to the light-sampling stream
     * (raygen.cu:625-628), which correlates the first path of every core with its own light sample.
     * Harmless at 100 paths per core (1 % of paths), a measured +1.5 % image bias at one path per core.
     * 1 = the BSDF stream starts from tea<4>(core ^ 0x80000000, frame) instead. */
    int32_t decorrelate_bsdf_stream;
} spcbpt_light_trace_params;

/* One light vertex as exchanged between ranks / checked by tests.  Values of
 * the BDPTVertex fields the connection code reads (BDPTVertex.h:9-70); the
 * device layout is the library's own. 96 bytes. */
typedef struct spcbpt_light_vertex {
    float position[3];
    float pdf;
    float normal[3];
    float single_pdf;
    float flux[3];
    float rmis_pointer;
    float color[3];
    float last_lum;
    float last_position[3];
    float last_normal_projection;
    int16_t material_id;
    int16_t subspace_id;
    int16_t depth;
    int16_t last_zone_id;
    uint32_t path_id;  /* global light path index = core * m_per_core + k */
    /* Cached classification: the vertex's label under the EYE tree + 1, written by the light pass for surface
     * vertices; 0 = not computed (an emitter vertex, or a cache the caller assembled: write 0).  The connection code uses
     * (pad & 0xffff) - 1 when that is a label (1 .. SPCBPT_NUM_SUBSPACE) and re-derives the label by a tree descent for any other value, so a
     * cache imported with a stale or uninitialised word costs time, never a wrong row of Gamma.  The label belongs to the
     * trees the cache was traced under (like subspace_id): trace a new cache after spcbpt_set_subspace. */
    uint32_t pad;
} spcbpt_light_vertex;
/* spcbpt_light_vertex::pad: bits 0-15 the cached eye-tree label + 1 (above); bit 31: the vertex is a direction of the environment
 * map (BDPTVertex::type == ENV: position = its point on the sky disk, normal = minus the sky direction); bit 30: the vertex was hit
 * straight from the environment map (BDPTVertex::isLastVertex_direction, hit_program.cu:412). */
#define SPCBPT_LV_DIRECTION 0x80000000u
#define SPCBPT_LV_LAST_DIRECTION 0x40000000u

/* Per-subspace record of the sampler = struct Subspace (optixPathTracer.h:43-51). */
typedef struct spcbpt_subspace {
    int32_t jump_bias;
    int32_t id;
    int32_t size;
    float sum_pmf;
    float q;
} spcbpt_subspace;

/* Event counters behind the algorithmic-bytes roofline. */
typedef struct spcbpt_counters {
    uint64_t closest_rays;
    uint64_t shadow_rays;
    uint64_t node_visits;
    uint64_t tri_tests;
    uint64_t surface_vertices;   /* closest hits that became path vertices */
    uint64_t textured_hits;
    uint64_t tree_nodes;         /* octree nodes visited by all classifications */
    uint64_t cmf_probes;         /* stage-1 + stage-2 binary-search probes */
    uint64_t connections;        /* light vertices fetched for connection */
    uint64_t gamma_q_reads;
    uint64_t lvc_stores;
    uint64_t pixel_samples;
    uint64_t eye_paths;
    uint64_t light_paths;
} spcbpt_counters;

typedef struct spcbpt_ctx spcbpt_ctx;

/* Replaces LoadScene + LightSource_shift + Scene_shift + sutil::Scene::finalize
 * (optixPathTracer.cpp:729-741; sutil/Scene.cpp:731-739: context, GAS, IAS,
 * modules, program groups, pipeline, SBT).  Uploads the scene and builds the
 * software LBVH.  device = HIP device ordinal.  The geometry is checked first, before a device is asked for:
 * SPCBPT_ERR_INVALID_ARG (text: spcbpt_last_error(NULL), naming the first offender) for a vertex coordinate, light corner
 * or light edge that is NaN or infinite and for a vertex index >= n_vertices; spcbpt_create_lit does the same. */
int spcbpt_create(const spcbpt_scene_desc* scene, int device, spcbpt_ctx** out);

/* Mesh lights: emissive meshes as area lights.  The reference routes every mesh whose material has |emissive_factor| > 0 to its
 * emitter hit programs (sutil/Scene.cpp:1739-1743) but has no light sampler for it (lightSample, cuProg.h:554-666, knows QUAD and
 * ENV), so those programs read a light id nobody set; this completes the route.  One mesh light = all triangles of the scene that
 * carry `material`, emitting the constant radiance `emission` from their front side -- the side normalize((P1-P0) x (P2-P0)) points
 * to -- exactly like a quad: single-sided for path rays, opaque to shadow rays, a path that hits it ends.  It is ONE entry of the
 * light list (after the quads, before the environment map; lights are picked uniformly); inside it a triangle is drawn in
 * proportion to its area and a point uniformly on it, so its point density is 1 / (sum of the triangle areas).  n_patches >= 1
 * emitter subspaces come from the same budget as the quads' div_level^2 (200 in all, 100 with an environment map): the triangles
 * are ordered along a Morton curve of their centroids and cut into n_patches runs of about equal area (fewer if the light has
 * fewer triangles).  Triangles without area are left out (they stay ordinary surface of `material`).  emissive textures,
 * two-sided emitters and a power-weighted choice between lights are not built. */
typedef struct spcbpt_mesh_light {
    int32_t material;   /* index into spcbpt_scene_desc::materials */
    float emission[3];
    int32_t n_patches;
} spcbpt_mesh_light;
/* spcbpt_create with mesh lights; scene->n_lights may be 0 when n_mesh_lights >= 1.  SPCBPT_ERR_INVALID_ARG (text: spcbpt_last_error(NULL))
 * for no light at all, a material out of range / named twice / used by no triangle, n_patches < 1, more than 200 patches in all,
 * or a light none of whose triangles has area.  spcbpt_create itself and spcbpt_scene_desc are unchanged. */
int spcbpt_create_lit(const spcbpt_scene_desc* scene, const spcbpt_mesh_light* mesh_lights, int n_mesh_lights, int device, spcbpt_ctx** out);
/* sizeof(spcbpt_mesh_light) as the library was compiled (spcbpt_abi_struct_sizes keeps its 13 entries). */
int spcbpt_mesh_light_struct_size(void);
/* One entry of the context's light list = params.lights (scene_shift.cpp:108-153: quads, then the environment map; here the mesh
 * lights that complete sutil/Scene.cpp:1739-1743 sit between them): type 0 QUAD / 1 ENV / 2 MESH, emitting area (0 for
 * ENV), emitting triangles, the label of its first patch subspace (patch k has label first_subspace - k) and the number of patches.
 * Any pointer may be NULL; SPCBPT_ERR_INVALID_ARG when `light` is not in [0, n_lights) (n_lights: spcbpt_get_environment). */
int spcbpt_light_info(spcbpt_ctx* ctx, int light, int32_t* type, float* area, int32_t* n_triangles, int32_t* first_subspace, int32_t* n_patches);
/* The sampling table spcbpt_create_lit builds for ONE mesh light (what lightSample, cuProg.h:554-666, would need for the emitters of
 * sutil/Scene.cpp:1739-1743 and does not have), without a device: `indices` = 3 x n_triangles vertex indices of the
 * light's triangles.  Outputs (n_triangles entries of capacity each, any may be NULL), in the order of the table: the input triangle,
 * its running area fraction (accumulated in double, the last exactly 1), its patch, its area; the summed area; the patches in use.
 * Returns the number of table entries (triangles with area; 0 = a degenerate light) or a negative spcbpt_status. */
int spcbpt_mesh_light_table(const float* vertices, int n_vertices, const uint32_t* indices, int n_triangles, int n_patches,
                            int32_t* tri_out, float* cmf_out, int32_t* patch_out, float* tri_area_out, double* area_out, int* n_patches_out);

/* Frees everything the context owns (the reference never frees). */
int spcbpt_destroy(spcbpt_ctx* ctx);

/* Last error text for this context (or for a failed create when ctx is NULL). */
const char* spcbpt_last_error(const spcbpt_ctx* ctx);

/* Replaces handleCameraUpdate: params.eye + Camera::UVWFrame
 * (optixPathTracer.cpp:352-370; sutil/Camera.cpp:34-45). */
int spcbpt_set_camera(spcbpt_ctx* ctx, const float eye[3], const float U[3],
                      const float V[3], const float W[3]);

/* Convenience: derive U,V,W exactly as sutil::Camera::UVWFrame does. */
int spcbpt_set_camera_lookat(spcbpt_ctx* ctx, const float eye[3], const float lookat[3],
                             const float up[3], float fov_y_deg, float aspect);

/* Replaces the accum_buffer allocation + params.width/height
 * (optixPathTracer.cpp:260-265, 319-333).  Clears accumulation. */
int spcbpt_resize(spcbpt_ctx* ctx, int width, int height);

/* Replaces subspaceInfo.{eye_tree, light_tree, Q, CMFGamma} assignment
 * (optixPathTracer.cpp:569-572, 606-607).  q has 1000 entries, cmf_gamma
 * 1000*1000 (row = eye subspace, inclusive CMF over light subspaces).
 * Passing all-NULL installs the minimal valid tuple of SURVEY.md 7 step 8
 * (single-leaf trees, Gamma rows proportional to Q estimated from light
 * passes) instead of the reference's biased null-tree fallback. */
int spcbpt_set_subspace(spcbpt_ctx* ctx,
                        const spcbpt_tree_node* eye_tree, int n_eye,
                        const spcbpt_tree_node* light_tree, int n_light,
                        const float* q, const float* cmf_gamma);

/* Replaces lt_params_setup (optixPathTracer.cpp:462-477). */
int spcbpt_set_light_trace(spcbpt_ctx* ctx, const spcbpt_light_trace_params* p);

/* A fifth launch name, "SPCBPT_no_rmis": the raygen program __raygen__SPCBPT_no_rmis (raygen.cu:445-606) exists in the
 * reference but is bound to no program group, so switchRaygen cannot select it there.  Same call sequence as "SPCBPT_eye"
 * ("light trace" -> spcbpt_build_sampler -> launch); the connections are weighted with classic full-path MIS
 * (contriCompute / pdfCompute / MISWeight_SPCBPT, cuProg.h:901-1105) instead of the recursive weights of rmis.h, and paths
 * longer than MAX_PATH_LENGTH_FOR_MIS = 20 vertices are dropped, as written.  A validation mode (one lane per pixel-sample, the
 * path in scratch memory, O(n^2) per connection): an independent estimator of the image "SPCBPT_eye" renders. */
/* Replaces switchRaygen(name) + optixLaunch (see file header).  name is one of
 * "pt", "light trace", "SPCBPT_eye", "pretrace".  For "pt" and "SPCBPT_eye"
 * frame is params.subframe_index; the image is cut into bands of 8 rows and
 * the rows y in [row_begin, row_end) with ((y/8 - row_begin/8) % row_step) == 0
 * are rendered: (0, height, 1) = whole image; rank r of N passes
 * (8*r, height, N) and gets every N-th band.  row_begin must be a multiple of
 * 8.  For "light trace" frame is lt_params.launch_frame
 * and the row arguments are ignored.  For "pretrace" frame is
 * pr_params.iteration.  Asynchronous.  "pretrace" draws its next-event point among the area lights (quad and mesh lights, never
 * the environment map) and its records claim that density, 1 / (area * number of area lights); without an area light it returns
 * SPCBPT_ERR_STATE.
 *
 * A sixth launch name, "lt": light tracing, the BDPT strategy t = 1 that upstream disables (readme.md:27).  Every vertex of the
 * light-vertex cache is connected straight to the camera and added to the pixel it lands on (spcbpt_camera_splat below gives
 * pixel and importance; a shadow ray to the eye decides visibility; box filter; no MIS weight, it is the only strategy of its
 * image and no clamp is applied).  Same call sequence and preconditions as "SPCBPT_eye" -- film, camera, "light trace" ->
 * spcbpt_build_sampler -> launch, else SPCBPT_ERR_STATE -- except that the subspace tuple is not read; frame is the subframe index
 * and the row arguments select 8-row bands as above (a splat that lands outside them is discarded, so ranks with disjoint band
 * sets render a correctly sharded film from the same cache).  The image converges to what "pt" converges to.  Not with an
 * environment map (SPCBPT_ERR_STATE: the directly seen sky is not sampled by this estimator, and sky vertices have no position),
 * not in the deferred / batched launch forms.  In the default (atomic) mode the sum uses float atomics: films agree to rounding,
 * not bit for bit, between runs; spcbpt_set_splat_order below selects a sum in a fixed order instead.
 * Event counters are left untouched; the kernel-time span is "lt". */
int spcbpt_launch(spcbpt_ctx* ctx, const char* name, uint32_t frame,
                  int row_begin, int row_end, int row_step);

/* How "lt" sums the contributions of a pixel (no reference counterpart).  SPCBPT_SPLAT_ATOMIC, the default: three float atomics per
 * contribution, in order of arrival.  SPCBPT_SPLAT_ORDERED: a launch reads n = min(vertex_count, capacity) vertices of the cache;
 * vertex i yields at most one record (pixel_i, rgb_i) -- exactly when the atomic mode would have added it, with the same bits -- and
 * the launch's radiance at pixel p is, per channel, +0.0f plus rgb_i of every record with pixel_i == p in ASCENDING i, one float32
 * addition per record.  A pixel without a record is +0.0f.  From there the launch goes on as in the atomic mode (running mean by
 * subframe, moments, tone map).  The film is then the same bits on every run, on every band split and in every context that holds
 * the same cache.  Costs, per render stream in use: 32 B per vertex of the cache capacity plus a radix sort's temporary storage,
 * allocated at the first ordered launch, grow-only, released by switching back to the atomic mode and by spcbpt_destroy; a context
 * that never asks keeps its footprint and its launches.  Any other mode value: SPCBPT_ERR_INVALID_ARG; a deferred frame
 * outstanding: SPCBPT_ERR_STATE.  Switching back waits for the context's streams.  Every refusal of "lt" holds in both modes. */
enum { SPCBPT_SPLAT_ATOMIC = 0, SPCBPT_SPLAT_ORDERED = 1 };
int spcbpt_set_splat_order(spcbpt_ctx* ctx, int mode);
int spcbpt_get_splat_order(spcbpt_ctx* ctx, int* mode);
/* The records of the last ordered "lt" launch, in cache order: *count = n, and for i < n pixel[i] = y * width + x with rgb[3 i ..]
 * the contribution, or pixel[i] = -1 (rgb 0) where vertex i yields no record (culled, occluded, outside the launch's rows).  What
 * a caller needs who wants a reconstruction filter of their own.  Waits like spcbpt_read_accum.  SPCBPT_ERR_STATE if there has been
 * no ordered launch since the last spcbpt_resize (or since the mode went back to atomic); SPCBPT_ERR_CAPACITY if `capacity`
 * (records the arrays hold) is below n -- *count is still set, nothing else is written. */
int spcbpt_read_splat_records(spcbpt_ctx* ctx, float* rgb, int32_t* pixel, int capacity, int* count);
/* The ordered sum over caller arrays on the host: n records (rgb 3 floats each, pixel index), out_rgb 3 floats per pixel of a
 * width x height film; records whose pixel is negative or >= width * height are skipped.  The code k_lt_gather runs (float32, no
 * contraction); no context and no GPU needed.  SPCBPT_ERR_INVALID_ARG for a NULL pointer (rgb / pixel may be NULL when n == 0),
 * n < 0 or an empty film. */
int spcbpt_splat_sum_host(const float* rgb, const int32_t* pixel, int64_t n, int width, int height, float* out_rgb);

/* The camera as the end of a light sub-path: where `point` lands on a width x height film seen through (eye, U, V, W) -- any
 * frame spcbpt_set_camera accepts, orthogonal or not -- and the importance "lt" gives it.  With c = point - eye, D = U . (V x W):
 *   g  = c . (U x V) / D                 (g <= 0: behind the camera)
 *   dx = (c . (V x W) / D) / g           dy = (c . (W x U) / D) / g           (|dx| >= 1 or |dy| >= 1: outside)
 *   px = floor((dx + 1) / 2 width)       py = floor((dy + 1) / 2 height)      (row 0 at dy = -1, as the eye rays are generated)
 *   weight = width height |c / g|^3 / (4 |D|)                                  (the reciprocal solid angle of a pixel along c)
 * Returns 1 and fills the outputs (any may be NULL) if the point projects inside the image, 0 (nothing written) otherwise.  Host
 * code, float32, no context and no GPU needed: the function the splat kernel itself calls. */
int spcbpt_camera_splat(const float eye[3], const float U[3], const float V[3], const float W[3],
                        int width, int height, const float point[3],
                        float* dx, float* dy, int* px, int* py, float* weight);

/* Thin-lens camera: a finite aperture, i.e. depth of field.  Off by default (radius 0 = the pinhole: every launch then runs the
 * kernels it always ran and every film keeps its bits; `focus` is ignored).
 *   radius >= 0   lens radius in world units; the lens is the disc around `eye` in the plane spanned by U and V
 *   focus  > 0    depth of the plane in focus, in units of W (for spcbpt_set_camera_lookat: 1 = the plane through `lookat`)
 * A pixel sample (x + jx, y + jy) has dx, dy as for the pinhole and the focus point F = eye + focus (dx U + dy V + W); its lens point
 * is O = eye + radius (a U / |U| + b V / |V|), (a, b) the concentric map of two uniform numbers onto the unit disc; the ray is
 * (O, normalize(F - O)) with weight 1, so a pixel is the mean over its footprint and over the lens of the radiance along that ray (no
 * cos^4 factor: with radius -> 0 the pinhole's convention).  The two lens numbers are drawn from the pixel's stream right behind the
 * jitter's (at subframe 0 too).  "lt" connects cache vertex i to a lens point of its own (seed tea4(i, subframe), two numbers) with
 * the importance spcbpt_camera_splat_lens states.
 * With radius > 0: spcbpt_launch and spcbpt_launch_deferred of "SPCBPT_eye" (timed kernel), "pt" and "lt" render through the lens.
 * SPCBPT_ERR_STATE, with a message naming the lens, from the forms that have no lens kernel -- none renders a pinhole image silently:
 * spcbpt_launch_eye_batch, spcbpt_launch_adaptive, "SPCBPT_no_rmis", the counting variants (spcbpt_enable_counters, classifier trees
 * with direction nodes) and "SPCBPT_eye" under SPCBPT_ENV_EYE_SEES_SKY.  The light pass, the sampler build and pretrace / preprocess
 * keep the pinhole at `eye` (they shape the sampling, not the estimate); spcbpt_launch_features, the denoisers and the history
 * reprojection use the centre-of-lens ray: their depth and normal are those of the sharp image.  A radius that pushes lens points
 * through geometry is the caller's business.  The lens survives spcbpt_set_camera* and spcbpt_resize.
 * SPCBPT_ERR_INVALID_ARG for a non-finite value, a negative radius or a focus <= 0. */
int spcbpt_set_lens(spcbpt_ctx* ctx, float radius, float focus);
int spcbpt_get_lens(spcbpt_ctx* ctx, float* radius, float* focus);   /* either pointer may be NULL; (0, 0) before the first spcbpt_set_lens */
/* The eye side on the host: n samples, pixel xy[2 i], xy[2 i + 1], jitter and lens numbers two floats each -> origin and direction,
 * three floats each.  Float32, no context and no GPU needed: the function the kernels call.  radius 0: `eye` and the pinhole direction. */
int spcbpt_camera_lens_ray_host(const float eye[3], const float U[3], const float V[3], const float W[3], int width, int height, int n,
                                const int32_t* xy, const float* jitter, const float* lens, float radius, float focus,
                                float* origin, float* dir);
/* The light side on the host: n world points (three floats each), each seen through the lens point of its two lens numbers.  With
 * c = point - O and g = c . (U x V) / D (g <= 0: rejected), q = (focus / g) c reaches the point F where the line O -> point meets the
 * plane in focus; (dx, dy) and the pixel are those of F (outside the image: rejected), and
 *   weight = width height |q|^3 / (4 focus^2 |q . (U x V)|)
 * is the reciprocal solid angle, seen from O, of the pixel's footprint on that plane.  inside[i] = 1 and dxdy / pixel (two each) /
 * weight filled, or 0 (zeros, pixel -1); dxdy, pixel and weight may be NULL.  radius 0: spcbpt_camera_splat, bit for bit. */
int spcbpt_camera_splat_lens(const float eye[3], const float U[3], const float V[3], const float W[3], int width, int height, int n,
                             const float* points, const float* lens, float radius, float focus,
                             float* dxdy, int32_t* pixel, float* weight, int32_t* inside);
/* The numbers a kernel draws for the camera: out = (jx, jy, u1, u2).  with_jitter != 0: the stream of pixel index = y * width + x
 * (jitter 0.5 and no draw for it at subframe 0); with_jitter == 0: the stream of cache slot `index` of "lt" (jx = jy = 0.5). */
int spcbpt_lens_sample_host(uint32_t index, uint32_t subframe, int with_jitter, float out[4]);
/* Debug: the device's own lens rays of `subframe`, eight floats per pixel of the film (origin xyz, direction xyz, 0, 0), from the
 * device function the lens kernels call.  Synchronous; the film is not touched. */
int spcbpt_debug_lens_rays(spcbpt_ctx* ctx, uint32_t subframe, float* out8);

/* Replaces MyThrustOp::LVC_Process (cuda_thrust/device_thrust.cu:241-332):
 * builds cmfs / jump_buffer / Subspace[1000] / vertex_count / path_count from
 * the LVC currently held by the context, on the device. Asynchronous. */
int spcbpt_build_sampler(spcbpt_ctx* ctx);

/* Multi-GPU exchange of the compacted LVC shard (no reference counterpart: the
 * reference is single-GPU).  export: device pointer to the
 * shard (array of spcbpt_light_vertex) and a device pointer to its int32
 * count; capacity in vertices.  import: replace the context's LVC by `count`
 * vertices from a device (is_device != 0) or host buffer. */
int spcbpt_lvc_export(spcbpt_ctx* ctx, void** d_vertices, void** d_count, int* capacity);
int spcbpt_lvc_import(spcbpt_ctx* ctx, const void* vertices, int count, int is_device);
/* Capacity, in vertices, of the context's compact light-vertex caches (the reference allocates LVC_MAX_NUM padded slots once,
 * optixPathTracer.cpp:470-475; here the cache exists once per frame in flight -- `sets` buffer sets of capacity x 104 B each --
 * so it is sized from the cache a pass really produces).  Default (0): the first light pass after spcbpt_set_light_trace is
 * traced once more as a probe (host wait, start-up) and the sets hold 2 x its vertex count (scaled to num_core for a rank's
 * share), at most num_core x core_padding.  A later pass that does not fit is cut off and the next spcbpt_sync returns
 * SPCBPT_ERR_CAPACITY.  set_capacity(vertices > 0) fixes the size by hand (allocates at once; the sets never shrink);
 * environment: SPCBPT_LVC_CAPACITY.  INTEGRATION.md lists the resulting HBM footprint. */
int spcbpt_lvc_set_capacity(spcbpt_ctx* ctx, int vertices);
int spcbpt_lvc_get_capacity(spcbpt_ctx* ctx, int* vertices, int* sets);
/* The same exchange without host round trips (libspcbpt_mgpu's RCCL host, include/spcbpt_mgpu.h):
 *   spcbpt_lvc_export_on        hands out the oldest pending shard like spcbpt_lvc_export and makes `hip_stream` (the caller's
 *                               exchange stream) wait for the light pass that fills it -- the host does not.
 *   spcbpt_lvc_import_gathered  `shards` = world x shard_capacity vertices exactly as an all-gather of every rank's shard (padded
 *                               to shard_capacity) leaves them, `counts_all` = world x {vertex_count, path_count} (device int32).
 *                               A device kernel queued on `hip_stream` concatenates the shards in rank order into the set and
 *                               leaves the totals on the device; spcbpt_build_sampler then runs over the upper bound
 *                               min(world x shard_capacity, LVC capacity) with pad keys instead of reading a count back.  A
 *                               shard larger than shard_capacity raises a device flag: the next spcbpt_sync returns
 *                               SPCBPT_ERR_CAPACITY.
 *   spcbpt_film_pack_bands / spcbpt_film_unpack_bands   exchange 2: this rank's 8-row bands (band b with b % world == rank) as one
 *                               contiguous block of ceil(bands / world) x 8 x width float4, and back from the all-gathered
 *                               world x that block into a full width x height float4 image (`out_image`, device). */
int spcbpt_lvc_export_on(spcbpt_ctx* ctx, void* hip_stream, void** d_vertices, void** d_count, int* capacity);
int spcbpt_lvc_import_gathered(spcbpt_ctx* ctx, const void* shards, const void* counts_all, int world, int shard_capacity, void* hip_stream);
/* One exchange per light BATCH (spcbpt_launch_light_batch): export_batch_on packs the shards of the n_frames oldest pending passes
 * (only their filled part) and their count pairs into the caller's contiguous send buffer `send` (n_frames x shard_capacity
 * vertices) / `send_counts` (n_frames x 2 int32) on `hip_stream`, which waits on the device for those passes; after ONE all-gather
 * of each, import_gathered_batch concatenates every frame's shards into that frame's set with one kernel (rank q's block holds its
 * frames one after the other: frame k at (q n_frames + k) x shard_capacity, counts at 2 (q n_frames + k)) and leaves the sets as
 * n_frames single spcbpt_lvc_import_gathered calls would: n_frames spcbpt_build_sampler calls follow. */
int spcbpt_lvc_export_batch_on(spcbpt_ctx* ctx, void* hip_stream, int n_frames, void* send, void* send_counts, int shard_capacity);
int spcbpt_lvc_import_gathered_batch(spcbpt_ctx* ctx, const void* shards, const void* counts_all, int world, int n_frames, int shard_capacity, void* hip_stream);
int spcbpt_film_pack_bands(spcbpt_ctx* ctx, int rank, int world, void* packed, void* hip_stream);
int spcbpt_film_unpack_bands(spcbpt_ctx* ctx, int world, const void* packed_all, void* out_image, void* hip_stream);
int spcbpt_image_size(spcbpt_ctx* ctx, int* width, int* height);
/* The environment map as one more light (row f4; upstream "unfinished", readme.md:29 -- what its live code does is built):
 * env_params_setup (optixPathTracer.cpp:431-461) + the ENV entry of LightSource_shift (scene_shift.cpp:108-153).  `rgba` = width x
 * height RGBA floats as the .hdr file stores them (row 0 = top; spcbpt_hdr_load); the context keeps the row-flipped texture
 * HDRLoader::loadTexture makes and the sampling CMF envMapCMFBuild makes.  Light sub-paths then start on the sky with probability
 * 1 / n_lights (cuProg.h:611-666), "SPCBPT_eye" connects to sky vertices (raygen.cu:234-258, rmis.h:249-280) and "pt" samples the
 * sky by next-event estimation and shows it to primary rays (hit_program.cu:502-518, raygen.cu:687-697).  As upstream, an eye
 * SUB-PATH that leaves the scene sees nothing by default: spcbpt_set_environment_mode below opts in.  center / radius = sky.center / sky.r (upstream: centre and diagonal of the scene
 * box it computes); radius <= 0 or center == NULL: centre and diagonal of the true bounding box.  The quad lights'
 * patch subspaces move up by 100 (their div_level^2 may sum to 100 at most).  Call once, before the first light pass.
 * Refused with SPCBPT_ERR_INVALID_ARG (the context stays as it was): more than 2^26 texels, a non-finite texel, an image without
 * energy, and a map too large for the float sampling table -- the table is accumulated in float as upstream's, and once an entry
 * does not exceed the one before it that texel would never be drawn although it shines (next-event estimation would lose its light);
 * the message names the first such texel.  (A smooth 2048 x 1024 sky still builds; a 4096 x 2048 one loses 1.4 % of its texels.) */
int spcbpt_set_environment(spcbpt_ctx* ctx, const float* rgba, int width, int height, const float* center, float radius);
int spcbpt_get_environment(spcbpt_ctx* ctx, int* width, int* height, float center[3], float* radius, int* n_lights);
/* Opt-in corrections of the sky's strategies (default 0 = upstream's behaviour); flags take effect only while the context has an
 * environment map, so a sky-less context renders bit-identically whatever they are.  May be called before or after
 * spcbpt_set_environment.
 *   SPCBPT_ENV_EYE_SEES_SKY              an eye sub-path of "SPCBPT_eye" that leaves the scene sees the sky: the strategy
 *                                        rmis::light_hit_env (rmis.h:325-358) weights, which upstream never calls although the
 *                                        weights of the other sky strategies count it -- without it the image is biased dark
 *                                         and directly seen sky is black.  The flux multiplier of the eye vertex is
 *                                        taken towards the sky (upstream's copy has the sign of the emitter case, HISTORY q1).
 *                                        Event-counting eye launches (spcbpt_enable_counters, or classifier trees with direction
 *                                        nodes) then return SPCBPT_ERR_STATE: their kernels do not evaluate the strategy.
 *   SPCBPT_ENV_PT_SKY_SHADOW_ALONG_DIR   the shadow ray of "pt"'s sky sample ends at P + d 2r instead of upstream's P + d + 2r
 *                                        (the scalar added to every component, q18).
 * Unknown bits: SPCBPT_ERR_INVALID_ARG; a deferred frame outstanding: SPCBPT_ERR_STATE.  Waits for the context's streams; the
 * film is not touched. */
enum { SPCBPT_ENV_EYE_SEES_SKY = 1, SPCBPT_ENV_PT_SKY_SHADOW_ALONG_DIR = 2 };
int spcbpt_set_environment_mode(spcbpt_ctx* ctx, int flags);
int spcbpt_get_environment_mode(spcbpt_ctx* ctx, int* flags);
/* Radiance .hdr reader = HDRLoader (scene_shift.cpp:334-500): RGBE, flat or new-style RLE scanlines, "-Y h +X w" only.  rgba == NULL:
 * size query.  The fourth float of a texel is 0 (upstream leaves it unset). */
int spcbpt_hdr_load(const char* path, int* width, int* height, float* rgba, size_t capacity_floats);
/* The light-pass geometry in force (spcbpt_set_light_trace with core_count resolved; the defaults before any call). */
int spcbpt_get_light_trace(spcbpt_ctx* ctx, spcbpt_light_trace_params* out);
/* Host copy of the LVC in deterministic order (path_id, depth). */
int spcbpt_lvc_read(spcbpt_ctx* ctx, spcbpt_light_vertex* out, int capacity, int* count);

/* Host copies of the sampler tables (tests, checkpointing). */
int spcbpt_sampler_read(spcbpt_ctx* ctx, spcbpt_subspace* subspace /*1000*/,
                        float* cmfs, int32_t* jump, int capacity,
                        int* vertex_count, int* path_count);

/* accum_buffer (float4 per pixel, row 0 = bottom of the view) and the
 * tone-mapped sRGB frame (raygen.cu:430-442).  Device pointer variant for
 * RCCL exchange. */
int spcbpt_read_accum(spcbpt_ctx* ctx, float* rgba_out);
int spcbpt_read_frame(spcbpt_ctx* ctx, uint8_t* rgba8_out);
int spcbpt_accum_device_ptr(spcbpt_ctx* ctx, void** d_accum);
/* SPCBPT_ERR_STATE while a deferred frame is outstanding (its merge would land in the cleared film). */
int spcbpt_clear_accum(spcbpt_ctx* ctx);
/* The film as of the LAST QUEUED merge (what spcbpt_sync_film waits for): accum (float4 per pixel) and / or the tone-mapped frame
 * (either may be NULL).  Unlike spcbpt_read_accum / spcbpt_read_frame, which wait for every stream of the context, this does not
 * wait for launches queued behind that merge -- a frame being traced ahead (spcbpt_launch_deferred), light passes ahead. */
int spcbpt_read_film(spcbpt_ctx* ctx, float* accum_rgba_out, uint8_t* frame_rgba8_out);

/* First-hit feature buffers (no reference counterpart): what the primary ray of "pt" sees first, the guides an image-space
 * denoiser takes.  The ray is the film's: subframe 0 goes through the pixel centre, subframe k > 0 takes the jitter the film's
 * sample of that subframe took, so features and film share one pixel footprint.  The sample of a subframe:
 *   first hit               albedo.rgb                                   albedo.w (coverage)  normal.xyz                 depth (normal.w)
 *   surface                 base colour (texture: bilinear, wrap,        1                    geometric normal, turned   hit distance
 *                           pow 2.2 -- what the BSDF is evaluated with)                       against the ray
 *   emitter, front side     (1, 1, 1)                                    1                    the light's normal         hit distance
 *   emitter, back side      as a miss (path rays see emitters from the front only)
 *   miss (sky or nothing)   (1, 1, 1)                                    0                    (0, 0, 0)                  0
 * Two float4-per-pixel device buffers in the film's row order (row 0 = bottom of the view) hold the running means
 * lerp(prev, sample, 1 / (subframe + 1)) of these values as they stand (subframe 0 overwrites): coverage is albedo.w, the normal
 * is the un-normalised mean, depth the mean with zeros for misses; a miss carries albedo 1 so that radiance / albedo needs no
 * branch.  The rows are spcbpt_launch's 8-row bands; rows outside them are left alone.  The buffers are allocated (zeroed) at the
 * first feature launch after spcbpt_resize: a context that never asks for features keeps its footprint.  Needs film and camera,
 * and no deferred frame outstanding (else SPCBPT_ERR_STATE).  Asynchronous, ordered with the film merges like the merge of a
 * "pt" launch; the film is not touched, event counters are not charged, the kernel-time span is "features". */
int spcbpt_launch_features(spcbpt_ctx* ctx, uint32_t subframe, int row_begin, int row_end, int row_step);
/* Host copies of the two buffers (either may be NULL); waits like spcbpt_read_accum.  SPCBPT_ERR_STATE if no feature launch has
 * been made since the last spcbpt_resize. */
int spcbpt_read_features(spcbpt_ctx* ctx, float* albedo_rgba, float* normal_depth_rgba);

/* Edge-avoiding a-trous wavelet denoiser (Dammertz et al. 2010) on the demodulated film, guided by the feature buffers.  With
 *   c_0(p) = accum(p).rgb / max(albedo(p).rgb, 1e-3) per channel,   n(p) = normal_depth(p).xyz,   X(p) = d_c(p) normal_depth(p).w
 *   (d_c: the normalised ray direction through the centre of pixel p),   L(c) = 0.3 r + 0.6 g + 0.1 b,
 * iteration i = 0 .. iterations - 1 with step s = 2^i runs over the taps q = p + s (a, b), a, b in -2 .. 2, inside the image:
 *   w(p, q) = k[a] k[b] exp(- |c_i(q) - c_i(p)|^2 / ((sigma_c 2^-i)^2 (1e-2 + (L(c_i(p)) + L(c_i(q))) / 2)^2)
 *                           - |n(q) - n(p)|^2 / sigma_n^2  -  |X(q) - X(p)|^2 / (sigma_x s)^2),     k = (1, 4, 6, 4, 1) / 16
 *   c_{i+1}(p) = sum_q w c_i(q) / sum_q w
 * and denoised(p).rgb = c_last(p) max(albedo(p).rgb, 1e-3), w = 1.  Smooth weights only: no threshold, no division by a guide.
 * iterations must be in 1 .. 8 (SPCBPT_ERR_INVALID_ARG); a sigma <= 0 selects its default: SPCBPT_DENOISE_SIGMA_C,
 * SPCBPT_DENOISE_SIGMA_N, and for sigma_x (a length in scene units) SPCBPT_DENOISE_SIGMA_X_FRACTION of the diagonal of the
 * scene's bounding box: (4, 1, 0.03), the triple with the lowest RMSE of a 4-frame Cornell box on the grid {1, 2, 4} x
 * {0.25, 0.5, 1} x {0.01, 0.03, 0.1} (tools/denoise_grid.py). */
typedef struct spcbpt_denoise_params {
    int32_t iterations;
    float sigma_c, sigma_n, sigma_x;
} spcbpt_denoise_params;
#define SPCBPT_DENOISE_SIGMA_C 4.0f
#define SPCBPT_DENOISE_SIGMA_N 1.0f
#define SPCBPT_DENOISE_SIGMA_X_FRACTION 0.03f
int spcbpt_denoise_params_struct_size(void);   /* sizeof(spcbpt_denoise_params) as the library was compiled (spcbpt_abi_struct_sizes keeps its 13 entries) */
/* Denoises the film as of every merge queued so far into a float4 buffer and an RGBA8 frame (the film's tone map) of its own;
 * accum and frame are not touched.  Needs a film, a feature launch since the last spcbpt_resize and no deferred frame
 * outstanding (else SPCBPT_ERR_STATE, with text).  Asynchronous; the kernel-time span is "denoise". */
int spcbpt_denoise(spcbpt_ctx* ctx, const spcbpt_denoise_params* params);
/* Waits for it and copies the result (either pointer may be NULL).  SPCBPT_ERR_STATE if nothing was denoised since the last resize. */
int spcbpt_read_denoised(spcbpt_ctx* ctx, float* rgba, uint8_t* rgba8);
/* The same filter on caller buffers on the host: float4-per-pixel accum, albedo and normal_depth as the read-backs give them, the
 * camera of spcbpt_set_camera (eye is accepted for symmetry: X enters through differences only).  No context and no GPU needed:
 * the per-pixel function the kernels run, float32, no contraction.  Without a scene the default of sigma_x is
 * SPCBPT_DENOISE_SIGMA_X_FRACTION of the bounding-box diagonal of the covered pixels' X.  The inputs are not written.
 * SPCBPT_ERR_INVALID_ARG for a NULL pointer, an empty image or iterations outside 1 .. 8. */
int spcbpt_denoise_host(const float* accum_rgba, const float* albedo_rgba, const float* normal_depth_rgba,
                        const float eye[3], const float U[3], const float V[3], const float W[3],
                        int width, int height, const spcbpt_denoise_params* params, float* out_rgba);

/* Reflected guides (no reference counterpart), opt-in: a second pair of guide planes in the layout of the first-hit feature buffers,
 * for which the primary ray is followed through mirror-like surfaces to the first surface that is not one.  A smooth metal shows its
 * own albedo, normal and depth in the first-hit planes, so a denoiser guided by them filters what the mirror reflects as if it were
 * irradiance on one flat surface; guided by these planes it sees the edges of the reflected scene.
 * Per pixel-sample (the ray of spcbpt_launch_features: camera_ray with the film's seed and subframe, from the centre of the lens),
 * with throughput (1, 1, 1), length 0 and the segments traced over (SPCBPT_SCENE_EPSILON, 1e16) like path rays:
 *   miss of the primary ray    albedo (1, 1, 1), coverage 0, normal 0, depth 0                  (the first-hit planes' miss)
 *   emitter, front side        albedo = throughput, coverage 1, the light's normal unfolded, depth = length + t
 *   emitter, back side         as a miss of that segment
 *   followed surface           a surface with roughness <= roughness_max && metallic >= metallic_min (false for a NaN), while fewer
 *                              than max_bounces mirrors have been followed:  throughput *= tint,  length += t,  on from the hit point
 *                              along R = dir - 2 (N.dir) N,  N the geometric normal turned against the ray;
 *                              tint = lerp(Cspec0, 1, schlick(|N.dir|)): the specular Fresnel colour of the BSDF at H = N
 *   any other surface          albedo = throughput x base colour (textured as in the first-hit planes), coverage 1, N unfolded,
 *                              depth = length + t
 *   miss of a later segment    the last mirror shows sky or void: albedo = throughput (that mirror's tint included), coverage 1, that
 *                              mirror's N unfolded through the mirrors before it, depth = the length up to that mirror
 * Unfolding carries a normal n found behind a mirror of normal N back through it, n - 2 (n.N) N, through all mirrors of the chain in
 * reverse order; depth is the unfolded path length.  The denoiser's position is eye + depth x primary direction: behind a planar
 * mirror that is the position of the virtual image, and the unfolded normal lives in the same space.  Curved mirrors work
 * approximately.  max_bounces = 0, or a roughness_max below every material's roughness, gives the first-hit planes bit for bit.
 * The three parameters are dials, not tuned against any image: the defaults follow up to 4 mirrors of roughness <= 0.1 and
 * metallic >= 0.9; a glossy dielectric (metallic 0) is mostly diffuse and stays with its own albedo. */
typedef struct spcbpt_guide_params {
    int32_t max_bounces;              /* 0 .. 8 */
    float roughness_max, metallic_min;
} spcbpt_guide_params;
#define SPCBPT_GUIDE_MAX_BOUNCES 4
#define SPCBPT_GUIDE_ROUGHNESS_MAX 0.1f
#define SPCBPT_GUIDE_METALLIC_MIN 0.9f
int spcbpt_guide_params_struct_size(void);   /* sizeof(spcbpt_guide_params) as the library was compiled */
/* One subframe's samples into the running means of the two guide planes (lerp(prev, sample, 1 / (subframe + 1)); subframe 0
 * overwrites), rows as in spcbpt_launch_features (8-row bands; rows outside them are left alone).  The planes are allocated (zeroed)
 * at the first guide launch after spcbpt_resize, which frees them.  SPCBPT_ERR_INVALID_ARG for NULL params, max_bounces outside
 * 0 .. 8, a NaN parameter or a row_begin that is not a multiple of 8; SPCBPT_ERR_STATE before spcbpt_resize, before a camera is set
 * and while a deferred frame is outstanding.  Asynchronous, a link of the film-merge chain like spcbpt_launch_features; no other
 * plane is touched, event counters are not charged, the kernel-time span is "guides". */
int spcbpt_launch_guides(spcbpt_ctx* ctx, uint32_t subframe, int row_begin, int row_end, int row_step, const spcbpt_guide_params* params);
/* Host copies of the two planes (either may be NULL); waits like spcbpt_read_accum.  SPCBPT_ERR_STATE if no guide launch has been
 * made since the last spcbpt_resize. */
int spcbpt_read_guides(spcbpt_ctx* ctx, float* albedo_rgba, float* normal_depth_rgba);
/* Which pair of planes spcbpt_denoise and spcbpt_denoise_variance take albedo and normal + depth from.  SPCBPT_GUIDES_FIRST_HIT (the
 * default): every call gives the bits it gave without this switch.  SPCBPT_GUIDES_REFLECTED: the guide planes; both denoisers then
 * refuse with SPCBPT_ERR_STATE (the text names spcbpt_launch_guides) if no guide launch has been made since the last spcbpt_resize.
 * Any other value: SPCBPT_ERR_INVALID_ARG.  The switch outlives spcbpt_resize.  spcbpt_history_capture / _reproject / _resolve /
 * _denoise and the adaptive calls keep the first-hit planes whatever it says: reprojection is the geometry of the first hit. */
#define SPCBPT_GUIDES_FIRST_HIT 0
#define SPCBPT_GUIDES_REFLECTED 1
int spcbpt_set_denoise_guides(spcbpt_ctx* ctx, int which);
/* The per-bounce arithmetic of the guide pass over host arrays, the functions the kernel runs (float32, no contraction; no context
 * and no GPU needed).  n records: dir and normal 3 floats each (the ray direction; the hit's unit normal turned against the ray),
 * material 6 floats (base r, g, b, metallic, roughness, specular) and specular_tint 1 float, test_normal 3 floats (a normal found
 * behind the mirror).  Out, each optional: followed (1 / 0: the roughness / metallic rule of `params`; max_bounces is not looked
 * at), reflected (R), tint and unfolded (the test normal carried back through the mirror), 3 floats per record.
 * SPCBPT_ERR_INVALID_ARG for a NULL input or n < 1. */
int spcbpt_guide_step_host(int64_t n, const float* dir, const float* normal, const float* material, const float* specular_tint,
                           const float* test_normal, const spcbpt_guide_params* params,
                           int32_t* followed, float* reflected, float* tint, float* unfolded);

/* Second moment of the film (no reference counterpart), opt-in: spcbpt_set_film_moments(ctx, 1).  Off (the default) a context keeps
 * its footprint, its launches and its film bits.  On, the context keeps one float4-per-pixel plane in the film's row order,
 *   m2n(p) = (M2_r, M2_g, M2_b, n),
 * and every film merge of spcbpt_launch ("pt", "SPCBPT_eye", "SPCBPT_no_rmis", "lt") and of spcbpt_merge_deferred(ctx, 1) is preceded
 * on its stream by an update of the pixels it is about to rewrite (the rows of the launch's 8-row bands), from the frame's sample x
 * and the mean before the merge, accum:
 *   subframe == 0:  M2 = 0, n = 1                                   (the film overwrites on subframe 0, so the moments restart)
 *   subframe  > 0:  a = 1 / (float)(subframe + 1),  mean' = mean + a (x - mean)   (the float operations of the merge: mean' is bit
 *                   M2 += (x - mean) (x - mean') per channel,  n += 1              for bit what the merge is about to store)
 * With subframes 0, 1, 2, ... in order this is Welford's update -- the assumption the film's own running mean makes; switched on
 * in mid-film, n counts the merges since.  A dropped deferred frame updates nothing.  The variance of the mean of channel k is
 * M2_k / (n (n - 1)) for n >= 2.  The plane (16 B per pixel) is allocated and zeroed at the first merge after spcbpt_resize, freed
 * by spcbpt_resize and by switching off (which waits for the context's streams), zeroed by spcbpt_clear_accum.  While the switch is on
 * spcbpt_launch_eye_batch returns SPCBPT_ERR_STATE (its merge takes up to 32 frames per pixel in one pass and keeps no moments;
 * spcbpt_launch_eye_batch_film is the batched launch whose merge keeps them);
 * the N-GPU host (spcbpt_mgpu.h) and the viewer do not use the switch.  The kernel-time span of the updates is "moments". */
int spcbpt_set_film_moments(spcbpt_ctx* ctx, int enabled);
int spcbpt_get_film_moments(spcbpt_ctx* ctx, int* enabled);
/* Host copy of the plane (zeros before the first merge); waits like spcbpt_read_accum.  SPCBPT_ERR_STATE while the switch is off. */
int spcbpt_read_film_moments(spcbpt_ctx* ctx, float* m2n_out);
/* One update of n_pixels pixels on the host: the per-pixel function the kernel runs (float32, no contraction) on float4-per-pixel
 * arrays -- the film before the merge, the frame's samples, and the plane, updated in place.  No context and no GPU needed.
 * SPCBPT_ERR_INVALID_ARG for a NULL pointer or n_pixels outside 1 .. 2^28. */
int spcbpt_film_moments_update_host(const float* mean_before_rgba, const float* sample_rgba, uint32_t subframe, int64_t n_pixels,
                                    float* m2n_inout);

/* Film error: how converged the film is.  The relative standard error of a pixel with n >= 2,
 *   e(p) = (0.3 sd_r + 0.6 sd_g + 0.1 sd_b) / (1e-2 + L(accum(p))),   sd_k = sqrt(max(M2_k, 0) / (n (n - 1))),   L = 0.3 r + 0.6 g + 0.1 b
 * -- the channels taken as fully correlated (an upper bound), the film's luminance weights, the denoiser's floor of 1e-2 -- reduced
 * over the pixels with n >= 2: their number, the mean and the maximum of e (pixels == 0: mean = max = 0).  Per-pixel terms in
 * float32, summed in double; per wave a fixed shuffle tree, per block through LDS, the blocks' partials added in index order by a
 * second one-block launch: no atomics, so two calls on the same film return the same bits.  Waits for the merges queued so far
 * and reads 24 bytes back.  SPCBPT_ERR_STATE while the moments are off.  The kernel-time span is "film_error". */
typedef struct spcbpt_film_error_stats {
    int64_t pixels;
    double mean, max;
} spcbpt_film_error_stats;
int spcbpt_film_error_struct_size(void);   /* sizeof(spcbpt_film_error_stats) as the library was compiled (spcbpt_abi_struct_sizes keeps its 13 entries) */
int spcbpt_film_error(spcbpt_ctx* ctx, spcbpt_film_error_stats* out);
/* The same over caller arrays on the host (float4 per pixel each), pixels in index order.  SPCBPT_ERR_INVALID_ARG as above. */
int spcbpt_film_error_host(const float* accum_rgba, const float* m2n, int64_t n_pixels, spcbpt_film_error_stats* out);

/* Bucket film (no reference counterpart), opt-in: spcbpt_set_film_buckets(ctx, K) with K = 0 (off, the default) or 3 .. 32.  Off, a
 * context keeps its footprint, its launches and its film bits.  On, the context keeps K float4 planes in the film's row order,
 * bucket-major [K][height][width],
 *   bucket_b(p) = (mean_r, mean_g, mean_b, n),
 * and every film merge of spcbpt_launch ("pt", "SPCBPT_eye", "SPCBPT_no_rmis", "lt") and of spcbpt_merge_deferred(ctx, 1) is preceded
 * on its stream by an update of the pixels it is about to rewrite (the rows of the launch's 8-row bands), from the frame's sample x,
 * into bucket b = subframe % K:
 *   subframe == 0:  every bucket of the pixel = (0, 0, 0, 0), then bucket 0 = (x, 1)   (the film overwrites on subframe 0, so the
 *                                                                                        buckets restart)
 *   subframe  > 0:  n' = n_b + 1,  a = 1 / n',  mean_b' = mean_b + a (x - mean_b) per channel,  n_b = n'
 * Independent of the moments switch; switched on in mid-film, the buckets count the merges since.  A dropped deferred frame updates
 * nothing.  The planes (16 K B per pixel) are allocated and zeroed at the first merge after spcbpt_resize, freed by spcbpt_resize
 * (K stays), by switching off and by changing K (both wait for the context's streams), zeroed by spcbpt_clear_accum.  While the
 * buckets are on, spcbpt_launch_eye_batch (its merge takes up to 32 frames per pixel in one pass and fills no buckets;
 * spcbpt_launch_eye_batch_film is the batched launch whose merge fills them) and spcbpt_adaptive_begin (its
 * per-tile merge fills no buckets) return SPCBPT_ERR_STATE with a text that names the buckets; while adaptive sampling is active,
 * spcbpt_set_film_buckets returns SPCBPT_ERR_STATE.  Any other K: SPCBPT_ERR_INVALID_ARG.  The N-GPU host (spcbpt_mgpu.h), the
 * viewer and the checkpoints do not use the switch.  The kernel-time span of the updates is "buckets". */
int spcbpt_set_film_buckets(spcbpt_ctx* ctx, int buckets);
int spcbpt_get_film_buckets(spcbpt_ctx* ctx, int* buckets);
/* Host copy of the K planes, K x height x width x 4 floats (zeros before the first merge); waits like spcbpt_read_accum.
 * SPCBPT_ERR_STATE while the buckets are off. */
int spcbpt_read_film_buckets(spcbpt_ctx* ctx, float* out);
/* One update of n_pixels pixels on the host: the per-pixel function the kernel runs (float32, no contraction) on the frame's samples
 * (float4 per pixel) and the planes [buckets][n_pixels] float4, updated in place.  No context and no GPU needed.
 * SPCBPT_ERR_INVALID_ARG for a NULL pointer, buckets outside 3 .. 32 or n_pixels outside 1 .. 2^28. */
int spcbpt_film_buckets_update_host(const float* sample_rgba, uint32_t subframe, int buckets, int64_t n_pixels, float* planes_inout);

/* Robust resolve: a median of means over the pixel's buckets that trims as much as the buckets disagree.  Per pixel, float32, no
 * contraction, every sum over the buckets in ascending index:
 *   live buckets: n_i > 0, k of them (k == 0: the output is (0, 0, 0, 0));   y_i = 0.3 r_i + 0.6 g_i + 0.1 b_i
 *   rank_i = the number of live j with y_j < y_i, or y_j == y_i and j < i
 *   T = sum y_i,   N = sum (float)(2 rank_i - k + 1) y_i
 *   G = 0 if k < 3 or !(T > 0), else N / ((float)k T) clamped to [0, 1]       (the Gini coefficient of the bucket luminances)
 *   t = ((strength G) (float)k) 0.5f,   d = min((k - 1) / 2, (int)floorf(t))
 *   kept: d <= rank_i < k - d;   rgb = sum n_i mean_i / sum n_i over the kept buckets;   w = (float)(k - 2 d)
 * The output plane holds (r, g, b, w).  G = 0 (all buckets agree, or strength = 0) gives the film's mean, G -> (k - 1) / k (one
 * bucket holds everything) the median bucket or buckets.  The estimator is BIASED wherever a pixel's true distribution is skewed:
 * a symmetric trim of the bucket means of a right-skewed variable darkens it; strength is the dial and 0 is the film.
 * The robust image is for display and for driving decisions; it does not replace accum.
 * spcbpt_robust_resolve writes a float4 plane and its RGBA8 tone map (the film's), read by spcbpt_read_robust (either pointer may be
 * NULL; it waits like spcbpt_read_accum; SPCBPT_ERR_STATE before the first resolve since spcbpt_resize / spcbpt_set_film_buckets).
 * It is a link of the film-merge chain like spcbpt_denoise and leaves accum, frame, the buckets and the moments untouched.  With the
 * buckets on but no merge yet the output is zeros (tone-mapped: opaque black).  strength must be a number in [0, 8], otherwise
 * SPCBPT_ERR_INVALID_ARG; SPCBPT_ERR_STATE while the buckets are off, before spcbpt_resize or while a deferred frame is outstanding.
 * The kernel-time span is "robust_resolve". */
int spcbpt_robust_resolve(spcbpt_ctx* ctx, float strength);
int spcbpt_read_robust(spcbpt_ctx* ctx, float* rgba, uint32_t* frame);
/* The same resolve over caller arrays on the host: planes [buckets][n_pixels] float4 as spcbpt_read_film_buckets gives them, out_rgba
 * float4 per pixel.  SPCBPT_ERR_INVALID_ARG for a NULL pointer, buckets outside 3 .. 32, n_pixels outside 1 .. 2^28 or a strength
 * outside [0, 8]. */
int spcbpt_robust_resolve_host(const float* planes, int buckets, int64_t n_pixels, float strength, float* out_rgba);

/* Display transform (no reference counterpart), opt-in: exposure, histogram auto-exposure and a choice of tone operators, written as
 * RGBA8 into a plane of its own.  accum, frame and every *_frame plane keep their bits; a context that never calls it keeps its
 * footprint and its launches.  Per pixel, float32, no contraction:
 *   L = 0.3 r + 0.6 g + 0.1 b
 *   histogram: 256 bins over the 32 octaves [2^-16, 2^16), eight per octave, cut from L's bit pattern:
 *     bin = (bits(L) >> 20) - ((127 - 16) << 3);   counter 256 `dark`: everything that is not >= 2^-16 (zero, negatives, NaN);
 *     counter 257 `bright`: everything >= 2^16 (+inf included).  258 uint32 counters, their sum is the pixel count.
 *   auto EV (double, only + - x /, so the device returns the host's bits): over the N in-range samples in ascending order drop the lowest
 *     (uint64)(low_fraction N) and the highest (uint64)(high_fraction N) -- a bin may be cut partially --, mean = the count-weighted mean
 *     of the kept bins' centres in log2, e + log2(1 + (m + 0.5) / 8);  target = clamp(log2(key) - mean + ev_bias, ev_min, ev_max);
 *     EV = prev + adapt (target - prev) with a previous EV, else target.  No in-range pixel: EV = prev, or clamp(ev_bias) without one.
 *   c' = c 2^EV, then the operator `op`:
 *     SPCBPT_TONE_FILM      c' / (1 + L' / 1.5)                       (the curve of spcbpt_read_frame, operation for operation)
 *     SPCBPT_TONE_REINHARD  c' (1 + L' / white^2) / (1 + L')
 *     SPCBPT_TONE_ACES      (x (2.51 x + 0.03)) / (x (2.43 x + 0.59) + 0.14) per channel
 *     SPCBPT_TONE_LINEAR    c'
 *   then clamp to [0, 1], sRGB, 8 bits, alpha 255.  The RGBA8 of a pixel with a non-finite channel is unspecified beyond alpha 255.
 * The adaptation state (the last auto EV and whether there is one) lives on the device: the exposure is computed by a kernel between the
 * histogram and the tone map and the pass never waits for the host.  A call with manual exposure neither reads nor writes that state. */
enum { SPCBPT_TONE_FILM = 0, SPCBPT_TONE_REINHARD = 1, SPCBPT_TONE_ACES = 2, SPCBPT_TONE_LINEAR = 3 };
enum { SPCBPT_DISPLAY_AUTO = 1,          /* EV from the image's histogram (`ev` is ignored) */
       SPCBPT_DISPLAY_HISTOGRAM = 2 };   /* compute the histogram under manual exposure too, for spcbpt_read_display */
enum { SPCBPT_DISPLAY_FILM = 0, SPCBPT_DISPLAY_DENOISED = 1, SPCBPT_DISPLAY_ROBUST = 2, SPCBPT_DISPLAY_HISTORY = 3,
       SPCBPT_DISPLAY_BLOOM = 4,         /* spcbpt_display and spcbpt_local_tone only: the bloom plane (spcbpt_bloom, below) */
       SPCBPT_DISPLAY_LOCAL = 5 };       /* spcbpt_display only: the local tone plane (spcbpt_local_tone, below) */
typedef struct spcbpt_display_params {
    int32_t op;                           /* SPCBPT_TONE_* */
    uint32_t flags;                       /* SPCBPT_DISPLAY_AUTO | SPCBPT_DISPLAY_HISTOGRAM */
    float ev;                             /* manual exposure, in stops */
    float key;                            /* auto: the luminance the trimmed log-mean is mapped to (> 0) */
    float low_fraction, high_fraction;    /* auto: the shares of the in-range pixels dropped from the dark / bright end; each in [0, 1), sum < 1 */
    float ev_bias, ev_min, ev_max;        /* auto: added to the target; the target's range (ev_min <= ev_max) */
    float adapt;                          /* auto: the step towards the target when there is a previous EV, in (0, 1] */
    float white;                          /* SPCBPT_TONE_REINHARD: the luminance (after exposure) that maps to white (> 0) */
} spcbpt_display_params;
/* op FILM, flags 0, ev 0, key 0.18, fractions 0.05 / 0.02, ev_bias 0, ev range -16 .. 16, adapt 1, white 4 */
int spcbpt_display_default_params(spcbpt_display_params* params);
int spcbpt_display_params_struct_size(void);   /* sizeof(spcbpt_display_params) as the library was compiled (spcbpt_abi_struct_sizes keeps its 13 entries) */
/* The pass on one of the context's linear images: source SPCBPT_DISPLAY_FILM (accum), _DENOISED (the latest output of spcbpt_denoise /
 * spcbpt_denoise_variance / spcbpt_history_denoise), _ROBUST (spcbpt_robust_resolve), _HISTORY (spcbpt_history_resolve), _BLOOM (the
 * plane spcbpt_bloom / spcbpt_bloom_image left, at that plane's own size; SPCBPT_ERR_STATE naming spcbpt_bloom without one) or _LOCAL
 * (the plane spcbpt_local_tone / spcbpt_local_tone_image left, likewise; SPCBPT_ERR_STATE naming spcbpt_local_tone).  A link of
 * the film-merge chain like spcbpt_robust_resolve: it sees everything queued before it.  Manual exposure is one launch; auto is a memset
 * of the counters, the histogram, the exposure kernel and the tone map on one stream.  Writes only its own plane and record.
 * SPCBPT_ERR_INVALID_ARG: a source or op that does not exist, unknown flag bits, fractions outside [0, 1) or summing to >= 1,
 * ev_min > ev_max, adapt outside (0, 1], key or white not > 0, a non-finite field.  SPCBPT_ERR_STATE, with a text that names what is
 * missing: the source image does not exist (no denoise / robust resolve / history resolve since it was last freed), before
 * spcbpt_resize, while a deferred frame is outstanding.  The kernel-time spans are "display_hist" (memset, histogram, exposure) and
 * "display" (the tone map). */
int spcbpt_display(spcbpt_ctx* ctx, int source, const spcbpt_display_params* params);
/* The same pass on an image the caller holds (float4 per pixel, any size up to 2^28 pixels): a PFM from disk, the film an N-GPU host
 * has gathered.  The image is copied to a scratch buffer of the context before the call returns; the adaptation state is the context's.
 * Needs no spcbpt_resize. */
int spcbpt_display_image(spcbpt_ctx* ctx, const float* rgba, int width, int height, const spcbpt_display_params* params);
/* What the last spcbpt_display / spcbpt_display_image left; every pointer may be NULL.  rgba8: width x height x 4 bytes of that call's
 * image size (ask for width / height first when it is not known); histogram258: 258 uint32; ev: the EV that was applied.  Waits like
 * spcbpt_read_accum.  SPCBPT_ERR_STATE before the first display call since spcbpt_resize, and for the histogram when the last call did
 * not compute one (manual exposure without SPCBPT_DISPLAY_HISTOGRAM). */
int spcbpt_read_display(spcbpt_ctx* ctx, uint8_t* rgba8, uint32_t* histogram258, float* ev, int* width, int* height);
/* Forgets the previous EV: the next auto call jumps to its target.  Ordered behind the display calls already queued.  spcbpt_resize
 * does the same and drops the display plane. */
int spcbpt_display_reset(spcbpt_ctx* ctx);
/* The same per-pixel code over caller arrays on the host: no context and no GPU needed.  have_prev / prev_ev: the adaptation state (read
 * under SPCBPT_DISPLAY_AUTO only).  rgba8_out (n_pixels x 4 bytes), histogram_out (258 uint32; filled whatever the flags) and ev_out
 * may each be NULL.  SPCBPT_ERR_INVALID_ARG as above, for NULL rgba / params and for n_pixels outside 1 .. 2^28. */
int spcbpt_display_host(const float* rgba, int64_t n_pixels, const spcbpt_display_params* params, int have_prev, float prev_ev,
                        uint8_t* rgba8_out, uint32_t* histogram_out, float* ev_out);

/* Bloom (no reference counterpart), opt-in: a multi-scale glare between the linear HDR image and the display transform.  A fraction
 * `strength` of the light above `threshold` leaves its pixel and is spread by a kernel that is a mix of `levels` near-Gaussian scales;
 * away from the image border light is neither created nor lost, so that a small emitter far above the key shows as a halo in proportion
 * to its power where the tone curve alone clips it to white.  The result is a float4 plane of its own at the source's size; accum,
 * frame and every *_frame plane keep their bits, and a context that never calls it keeps its footprint and its launches.
 * Per texel, float32, no contraction, r g b alike, alpha copied.  I is the source, W x H:
 *   1. C = I > 0 ? min(I, clamp) : 0  (NaN and negatives give 0, +inf gives clamp);  Y = 0.3 Cr + 0.6 Cg + 0.1 Cb;
 *      t = Y > threshold ? (Y - threshold) / Y : 0;  P = C t   (a ramp, continuous at the threshold; threshold 0: P = C)
 *   2. D_0 = P;  D_{k+1} is ceil(W_k / 2) x ceil(H_k / 2):  D_{k+1}(x, y) = sum_j sum_i w_j w_i D_k(cx(2x - 1 + i), cy(2y - 1 + j)),
 *      i, j = 0 .. 3, w = (1, 3, 3, 1) / 8, cx / cy clamp to the level's edge; the four horizontal sums first, each
 *      ((w0 a0 + w1 a1) + w2 a2) + w3 a3, then the same form down the column
 *   3. g_k = spread^(k-1) / sum_{m=1..L} spread^(m-1) (in double, rounded to float once);  U_L = g_L D_L;  U_k = g_k D_k + up(U_{k+1});
 *      B = up(U_1) at the source's size;  up(A)(x, y): px = x >> 1, nx = clamp(px + (x & 1 ? 1 : -1)), 0.75 A(px) + 0.25 A(nx)
 *      horizontally on the rows py and ny, then the same vertically over those two
 *   4. O = I + strength (B - P),  O_a = I_a.  What is above `clamp` stays where it was; a NaN stays in its channel of its pixel. */
typedef struct spcbpt_bloom_params {
    int32_t levels;       /* L, the scales of the pyramid: 1 .. 8 (a level never gets smaller than 1 x 1) */
    float strength;       /* s, the share of the light above the threshold that is redistributed: [0, 1] */
    float spread;         /* q, the weight of a level relative to the next finer one: (0, 4]; 1 weighs all levels alike */
    float threshold;      /* T, the luminance below which a pixel gives nothing: >= 0 */
    float clamp;          /* K, the most a channel may give: (0, 2^64] */
} spcbpt_bloom_params;
/* levels 5, strength 0.1, spread 1, threshold 0, clamp 65504 */
int spcbpt_bloom_default_params(spcbpt_bloom_params* params);
int spcbpt_bloom_params_struct_size(void);   /* sizeof(spcbpt_bloom_params) as the library was compiled (spcbpt_abi_struct_sizes keeps its 13 entries) */
/* The stage on one of the context's linear images: source SPCBPT_DISPLAY_FILM, _DENOISED, _ROBUST or _HISTORY, as spcbpt_display takes
 * them.  A link of the film-merge chain like spcbpt_display: it sees everything queued before it.  Writes only the context's bloom
 * plane and its pyramid scratch (float4 per texel of the levels 1 .. L, about a third of the image).  The launches: a tiled down pass
 * per fine level (level 0 with step 1 fused in), one workgroup that runs the coarse end of the pyramid down and back up in LDS, an up
 * pass per fine level, the composite; one kernel-time span, "bloom".  SPCBPT_ERR_INVALID_ARG, with a text that contains `bloom`: a
 * source that does not exist, a field outside its range above or not finite.  SPCBPT_ERR_STATE with spcbpt_display's texts: the source
 * image does not exist, before spcbpt_resize, while a deferred frame is outstanding. */
int spcbpt_bloom(spcbpt_ctx* ctx, int source, const spcbpt_bloom_params* params);
/* The same stage on an image the caller holds (float4 per pixel, 1 .. 2^28 pixels): the film an N-GPU host has gathered, a PFM from
 * disk.  The image is copied to a scratch buffer of the context before the call returns.  Needs no spcbpt_resize. */
int spcbpt_bloom_image(spcbpt_ctx* ctx, const float* rgba, int width, int height, const spcbpt_bloom_params* params);
/* The bloom plane the last spcbpt_bloom / spcbpt_bloom_image left: width x height float4 of that call's image size; every pointer may
 * be NULL (ask for width / height first when the size is not known).  Waits like spcbpt_read_accum.  SPCBPT_ERR_STATE before the first
 * bloom call since spcbpt_resize, which frees the plane and the pyramid (as spcbpt_destroy does). */
int spcbpt_read_bloom(spcbpt_ctx* ctx, float* rgba, int* width, int* height);
/* The same per-texel code over caller arrays on the host: no context and no GPU needed.  out_rgba: width x height float4, must not
 * overlap rgba.  SPCBPT_ERR_INVALID_ARG as above, for a NULL pointer and for an image outside 1 .. 2^28 pixels. */
int spcbpt_bloom_host(const float* rgba, int width, int height, const spcbpt_bloom_params* params, float* out_rgba);

/* Local tone mapping (no reference counterpart), opt-in: a base / detail decomposition of log-luminance through a bilateral grid
 * (Chen, Paris and Durand 2007; Durand and Dorsey 2002) between the linear HDR image -- or the bloom plane -- and the display
 * transform.  The large-scale luminance range of the image is compressed about `anchor`, local contrast is kept, and because the grid
 * separates pixels by luminance as well as by position a strong edge gets no halo: an interior lit by a small bright emitter keeps
 * both the lamp's wall and the far corner inside one exposure.  The result is a float4 plane of its own at the source's size; every
 * other plane keeps its bits, and a context that never calls it keeps its footprint and its launches.
 * Float32 per pixel and per grid node, no contraction; only + - x /, compares, int <-> float conversions and bit-pattern moves are on
 * the path, so the device plane equals spcbpt_local_tone_host bit for bit.  I is the source, W x H, s = cell, rho = range:
 *   1. Y = 0.3 r + 0.6 g + 0.1 b.  A pixel TAKES PART iff Y > 0 && Y < +inf (NaN, zero, negatives and infinities do not).  For those
 *      Yc = min(max(Y, 2^-16), 2^16) and L = lt_log2(Yc) in [-16, 16]:  lt_log2 = e + P(m - 1), e and m in [1, 2) cut from the bit
 *      pattern, P(t) = t + t (0.44183588 + t (-0.7083722 + t (0.41355506 + t (-0.19126251 + t 0.04424374)))), P(0) = 0 exactly.
 *      Its inverse lt_exp2(g): g clamped to [-32, 32], i = floor(g), f = g - i, Q(f) times the float with the bit pattern
 *      (i + 127) << 23, Q(f) = 1 + f (0.6930049 + f (0.24153961 + f (0.051766057 + f 0.013689456))), lt_exp2(0) == 1 exactly.
 *      |lt_log2 - log2| <= 1.8e-5 stops, |lt_exp2 / exp2 - 1| <= 4.6e-6 (the condition is 2^-13 for both); both are non-decreasing.
 *   2. The grid: GX = (W - 1) / s + 2, GY = (H - 1) / s + 2 (integer division), NZ = (int)(32 / rho) + 2 (the quotient in float32),
 *      two channels A, B per node; a pixel's bin coordinate is z = (L + 16) / rho.  More than 2^25 nodes: SPCBPT_ERR_INVALID_ARG.
 *      Node (gx, gy, gz) gathers the pixels that take part with |x - gx s| < s and |y - gy s| < s under the tents
 *      wx = (float)(s - |x - gx s|) / (float)s, wy likewise, wz = 1 - |z - (float)gz| where that is > 0, else 0.  The order of the sums
 *      is part of the definition: row sums, x ascending, a_j = sum (wx wz) L and b_j = sum (wx wz); then, rows ascending,
 *      A = sum wy_j a_j and B = sum wy_j b_j; each a plain left-to-right float32 sum from 0.  A gather, no atomics: deterministic.
 *   3. Blur, `blur` times: along x over the whole grid, then y, then z, both channels,
 *      out(i) = (0.25 v(i - 1) + 0.5 v(i)) + 0.25 v(i + 1), indices clamped to the grid.
 *   4. Slice, for a pixel that takes part: ix = x / s, tx = (float)(x - ix s) / (float)s, the same in y; iz = min((int)z, NZ - 2),
 *      tz = z - (float)iz; lerp(a, b, t) = a + t (b - a).  A and B separately: along z in each of the four columns, then along x in the
 *      rows iy and iy + 1, then along y.  base = A / B if B > 0, else L.
 *   5. g = (compress - 1)(base - La) + (detail - 1)(L - base), La = log2(anchor) taken in double and rounded to float once;
 *      O_rgb = I_rgb lt_exp2(g), O_a = I_a.  A pixel that takes no part keeps its four floats bit for bit; with compress = detail = 1
 *      the whole plane is the source bit for bit. */
typedef struct spcbpt_local_tone_params {
    int32_t cell;         /* s, pixels per grid cell: 4 .. 64 */
    float range;          /* rho, stops per grid bin: [0.5, 8] */
    int32_t blur;         /* grid blur passes: 0 .. 4 */
    float compress;       /* c, the slope of the base layer: (0, 2]; 1 leaves the large-scale range as it is */
    float detail;         /* d, the slope of the detail layer: [0, 4]; 1 leaves local contrast as it is */
    float anchor;         /* the luminance whose base stays put: > 0 */
} spcbpt_local_tone_params;
/* cell 16, range 1, blur 1, compress 0.5, detail 1, anchor 0.18 */
int spcbpt_local_tone_default_params(spcbpt_local_tone_params* params);
int spcbpt_local_tone_params_struct_size(void);   /* sizeof(spcbpt_local_tone_params) as the library was compiled (spcbpt_abi_struct_sizes keeps its 13 entries) */
/* The stage on one of the context's linear images: source SPCBPT_DISPLAY_FILM, _DENOISED, _ROBUST or _HISTORY as spcbpt_display takes
 * them, or _BLOOM: glare first, then the local operator.  The local plane itself is no source, of this stage or of spcbpt_bloom.  A
 * link of the film-merge chain like spcbpt_bloom: it sees everything queued before it.  Writes only the context's local tone plane and
 * its two grid buffers (two floats per node each).  The launches: the gather (one workgroup per node column), one launch per
 * blur pass (its three axes together), the slice with the gain; one kernel-time span, "local_tone".  SPCBPT_ERR_INVALID_ARG, with a text that contains
 * `local_tone`: a source that does not exist, a field outside its range above or not finite, a grid of more than 2^25 nodes.
 * SPCBPT_ERR_STATE with spcbpt_display's texts: the source image does not exist (naming spcbpt_bloom for _BLOOM), before
 * spcbpt_resize, while a deferred frame is outstanding. */
int spcbpt_local_tone(spcbpt_ctx* ctx, int source, const spcbpt_local_tone_params* params);
/* The same stage on an image the caller holds (float4 per pixel, 1 .. 2^28 pixels).  The image is copied to a scratch buffer of the
 * context before the call returns.  Needs no spcbpt_resize. */
int spcbpt_local_tone_image(spcbpt_ctx* ctx, const float* rgba, int width, int height, const spcbpt_local_tone_params* params);
/* The plane the last spcbpt_local_tone / spcbpt_local_tone_image left: width x height float4 of that call's image size; every pointer
 * may be NULL.  Waits like spcbpt_read_accum.  SPCBPT_ERR_STATE before the first call since spcbpt_resize, which frees the plane and
 * the grid buffers (as spcbpt_destroy does). */
int spcbpt_read_local_tone(spcbpt_ctx* ctx, float* rgba, int* width, int* height);
/* The same per-pixel and per-node code over caller arrays on the host: no context and no GPU needed.  out_rgba: width x height float4,
 * must not overlap rgba.  SPCBPT_ERR_INVALID_ARG as above, for a NULL pointer and for an image outside 1 .. 2^28 pixels. */
int spcbpt_local_tone_host(const float* rgba, int width, int height, const spcbpt_local_tone_params* params, float* out_rgba);
/* For the tests: lt_log2 (which = 0) or lt_exp2 (which = 1) of step 1 over n floats. */
int spcbpt_local_tone_math_host(const float* in, int64_t n, int which, float* out);

/* Adaptive sampling (no reference counterpart), opt-in: trace only the tiles of the film that are still above a target error.  A TILE
 * is an 8x8 pixel block of the whole film, numbered x-major: tile t covers x = (t % tiles_x) 8 ..., y = (t / tiles_x) 8 ... with
 * tiles_x = ceil(width / 8); edge tiles are partial.  The adaptive state of a context is a sample count per tile (uint32), an error
 * per tile (float) and a tile list (uint32, strictly ascending) with its length.
 *
 * spcbpt_adaptive_begin(ctx, frames) declares that the film holds the uniform subframes 0 .. frames - 1 (spcbpt_history_capture's
 * convention) and sets every tile's count to `frames` (0 is allowed); the list starts empty.  It needs the film's moments switched
 * on and no deferred frame outstanding (else SPCBPT_ERR_STATE), and waits for the context's streams.  While the mode is active every
 * call that merges into the film with one weight for all pixels -- spcbpt_launch of "pt", "SPCBPT_eye", "SPCBPT_no_rmis" and "lt",
 * spcbpt_launch_deferred, spcbpt_launch_eye_batch -- and spcbpt_set_film_moments(ctx, 0) return SPCBPT_ERR_STATE with a text that
 * names adaptive sampling; "light trace", "pretrace", the sampler builds, spcbpt_launch_features, the denoisers, the history calls,
 * spcbpt_film_error and every read work as before (they only read the film, and the moments plane carries each pixel's own n).
 * spcbpt_adaptive_end, spcbpt_resize and spcbpt_clear_accum end the mode and drop the counts; spcbpt_adaptive_end leaves the film as it is.
 *
 * spcbpt_adaptive_select computes, for every tile, e_t = the mean of e(p) (spcbpt_film_error's per-pixel term) over the tile's
 * pixels inside the image that have n >= 2 -- none: e_t = 0 and the tile is "unknown" -- and lists tile t, in ascending order, iff
 *   (max_samples == 0 || samples_t < max_samples)  &&  (samples_t < max(min_samples, 2) || t is unknown || e_t > target_error).
 * Float32; the 64 slot terms of a tile are added by halving (slot s + 32 to slot s, then + 16, ... + 1): one wave per tile, a fixed
 * shuffle tree, and one block that scans the tiles -- no atomics, so the same film gives the same bits.  The call waits for the merges
 * queued so far and for its own result, and returns the list's length in *n_selected (may be NULL).  The kernel-time span is
 * "adaptive_select".  A stopping rule that reads an estimate computed from the samples it stops biases the result slightly towards
 * early stops; min_samples is the guard.  Beyond that rule every sample is exactly the uniform renderer's.
 *
 * spcbpt_adaptive_set_tiles imposes a list instead (region rendering, tests): strictly ascending and in range, else
 * SPCBPT_ERR_INVALID_ARG; n = 0 is allowed.  It waits for the context's streams.
 *
 * spcbpt_launch_adaptive(ctx, "SPCBPT_eye") has the preconditions of spcbpt_launch(ctx, "SPCBPT_eye", ...) -- film, camera, a light
 * pass, a built sampler -- and traces ONE sample for every pixel of every listed tile: a pixel of tile t uses samples_t wherever an
 * ordinary launch uses its subframe (seed and jitter of the camera ray, the weight 1 / (samples_t + 1) of the running mean, the
 * subframe of the moments update: 0 restarts).  It then merges the listed tiles only and adds 1 to their counts.  Pixels of unlisted
 * tiles keep every bit of accum, frame and the moments plane; an empty list is a successful no-op.  Any other algorithm name:
 * SPCBPT_ERR_INVALID_ARG.  SPCBPT_ERR_STATE with event counters on, with SPCBPT_ENV_EYE_SEES_SKY set, or with classifier trees
 * that have direction nodes (the forms the timed kernels do not cover).  Asynchronous; the kernel-time spans are "adaptive_eye" and
 * "adaptive_merge".
 *
 * spcbpt_read_adaptive copies the counts and the errors of the last select ([tiles_y * tiles_x] each) and the list (at most `capacity`
 * entries; SPCBPT_ERR_INVALID_ARG if it holds more) to the host and leaves the list's length in *n; every pointer is optional.  It
 * waits like spcbpt_read_accum.  spcbpt_get_adaptive_state never waits (inactive: 0, 0, 0, 0). */
typedef struct spcbpt_adaptive_params {
    float target_error;     /* a tile whose mean relative standard error is above this is traced again */
    uint32_t min_samples;   /* every tile gets at least max(min_samples, 2) samples */
    uint32_t max_samples;   /* no tile gets more than this; 0 = no cap */
} spcbpt_adaptive_params;
int spcbpt_adaptive_params_struct_size(void);   /* sizeof(spcbpt_adaptive_params) as the library was compiled (spcbpt_abi_struct_sizes keeps its 13 entries) */
int spcbpt_adaptive_begin(spcbpt_ctx* ctx, uint32_t frames);
int spcbpt_adaptive_end(spcbpt_ctx* ctx);
int spcbpt_adaptive_select(spcbpt_ctx* ctx, const spcbpt_adaptive_params* params, int* n_selected);
int spcbpt_adaptive_set_tiles(spcbpt_ctx* ctx, const uint32_t* tiles, int n);
int spcbpt_launch_adaptive(spcbpt_ctx* ctx, const char* algorithm);
int spcbpt_read_adaptive(spcbpt_ctx* ctx, uint32_t* tile_samples, float* tile_error, uint32_t* tiles, int capacity, int* n);
int spcbpt_get_adaptive_state(spcbpt_ctx* ctx, int* active, int* tiles_x, int* tiles_y, int* n_listed);
/* The selection over caller arrays on the host (float4 per pixel each, tile_samples per tile): the per-tile functions the kernels run,
 * in their order.  tile_error_out ([tiles]), tiles_out ([tiles] at most) and n_out are optional.  No context and no GPU needed.
 * SPCBPT_ERR_INVALID_ARG for a NULL input pointer, a size outside 1 .. 2^28 pixels or a target that is not a number. */
int spcbpt_adaptive_select_host(const float* accum_rgba, const float* m2n, int width, int height, const uint32_t* tile_samples,
                                const spcbpt_adaptive_params* params, float* tile_error_out, uint32_t* tiles_out, int* n_out);

/* Variance-guided a-trous denoiser: the pipeline, guides, buffers and outputs of spcbpt_denoise (read with spcbpt_read_denoised),
 * with a colour weight measured in the pixel's own standard error instead of a fixed relative width -- so the filter narrows as
 * the film converges and becomes the identity in the limit, where spcbpt_denoise blurs a 4-frame and a 4000-frame film alike.
 * A scalar variance v of the demodulated luminance travels with c.  Start values (w = (0.3, 0.6, 0.1), sd_k as above):
 *   c_0(p) = accum(p).rgb / max(albedo(p).rgb, 1e-3)
 *   v_0(p) = (sum_k w_k sd_k / max(albedo_k(p), 1e-3))^2     for n(p) >= 2
 *          = L(c_0(p))^2                                     for n(p) <  2   (unknown variance: as uncertain as its own value)
 * Iteration i with step s = 2^i, taps q = p + s (a, b) inside the image, k = (1, 4, 6, 4, 1) / 16:
 *   v~_i(p) = the (1/4, 1/2, 1/4)^2 mean of v_i over the 3 x 3 neighbours of p at distance 1 inside the image, renormalised
 *   w(p, q) = k[a] k[b] exp(- (L(c_i(q)) - L(c_i(p)))^2 / (sigma_v^2 v~_i(p) + (1e-3 (1e-2 + L(c_i(p))))^2)
 *                           - |n(q) - n(p)|^2 / sigma_n^2  -  |X(q) - X(p)|^2 / (sigma_x s)^2)
 *   c_{i+1}(p) = sum_q w c_i(q) / sum_q w,      v_{i+1}(p) = sum_q w^2 v_i(q) / (sum_q w)^2
 * Smooth weights only; the single branch is on the integer n.  A pixel of zero variance merges only with neighbours within a
 * thousandth of its luminance; the centre tap keeps the sum non-empty.  spcbpt_denoise_params is reused: its sigma_c field is read
 * as sigma_v (<= 0: SPCBPT_DENOISE_SIGMA_V = 4, the one value of {2, 4, 8} that leaves the Cornell box closer to the converged image
 * than the film at 4 and at 64 frames: DESIGN.md 8e; tools/denoise_grid.py), sigma_n and sigma_x as in spcbpt_denoise.  Needs the moments switched on, a feature launch since the
 * last spcbpt_resize and no deferred frame outstanding (else SPCBPT_ERR_STATE, with text).  Asynchronous; the kernel-time span is
 * "denoise_variance". */
#define SPCBPT_DENOISE_SIGMA_V 4.0f
int spcbpt_denoise_variance(spcbpt_ctx* ctx, const spcbpt_denoise_params* params);
/* The same filter on caller buffers on the host (see spcbpt_denoise_host), with the moment plane as spcbpt_read_film_moments gives it. */
int spcbpt_denoise_variance_host(const float* accum_rgba, const float* m2n, const float* albedo_rgba, const float* normal_depth_rgba,
                                 const float eye[3], const float U[3], const float V[3], const float W[3],
                                 int width, int height, const spcbpt_denoise_params* params, float* out_rgba);

/* History reprojection (no reference counterpart), opt-in: the converged image of one camera carried into the next through the
 * first-hit depth, so that a camera move does not fall back to one sample per pixel.  The scene is static, so where a pixel was is
 * a function of its depth and of the two cameras; nothing else is kept.  A context that never calls these keeps its footprint, its
 * launches and its film bits; film, frame, features, moments and counters are never written.
 * A HISTORY is taken at capture time: a float4 plane H(q) = (rgb, n), the image and its effective frame count; a float4 plane G(q),
 * the normal / depth feature plane as it stood; the camera (eye_h, U_h, V_h, W_h); the film size.  A PRIOR is one float4 plane
 * R(p) = (rgb, m) in the current view, m the number of frames the prior is worth at p.
 * Reproject, for every pixel p = (x, y) of the current film, float32 without contraction, with nd = normal_depth(p):
 *   nd.w <= 0 (a miss):  R(p) = 0
 *   P = eye + X(p),  X(p) = d_c(p) nd.w as in the denoiser (the centre ray);   c = P - eye_h,   D = U_h . (V_h x W_h)
 *   g = c . (U_h x V_h) / D,   dx = (c . (V_h x W_h) / D) / g,   dy = (c . (W_h x U_h) / D) / g      (the algebra of camera_splat)
 *   g <= 0:  R(p) = 0
 *   fx = clamp((dx + 1) / 2 width - 0.5, -2, width + 1),  x0 = floor(fx),  ax = fx - x0;   fy, y0, ay likewise with height
 *   the four taps q = (x0 + i, y0 + j), i, j in {0, 1}; a tap outside the image or with G(q).w <= 0 has weight 0, else
 *   b_q = (i ? ax : 1 - ax) (j ? ay : 1 - ay),    X_q = eye_h + d_c,h(q) G(q).w
 *   w_q = b_q exp(-(nd.xyz . (X_q - P))^2 / sigma_x^2 - |G(q).xyz - nd.xyz|^2 / sigma_n^2)
 *   S = sum w_q,   C = sum w_q H(q).rgb,   N = sum w_q H(q).n
 *   S < 1e-6:  R(p) = 0,   else R(p) = (C / S, S min(N / S, max_history))
 * The weights are smooth and the floor is harmless (the bilinear weight of a tap is zero where it enters or leaves); the only
 * decisions on computed values are g <= 0, where every tap is outside anyway, and the S cut, a jump of at most 1e-6 frames -- so a
 * float64 evaluation agrees everywhere.  A disoccluded pixel finds taps on another surface: the plane distance and the normal
 * difference take its weight, m, to zero and the film alone shows there.
 * Resolve(frames), frames >= 1, Nf = (float)frames, m = R(p).w (0 where no prior is live):
 *   out(p).rgb = (m R(p).rgb + Nf accum(p).rgb) / (m + Nf),   out(p).w = m + Nf;   an RGBA8 plane holds the film's tone map of out.rgb
 * (while no prior is live out.rgb is accum.rgb bit for bit -- the value of the formula with m = 0, without its two roundings)
 * Capture(frames), frames >= 1: H becomes the resolve of the current film (a live prior is folded in, so a chain of moves keeps its
 * history), G a copy of the current normal_depth plane, the current camera is stored, and the prior stops being live.
 * A parameter <= 0 selects its default -- for sigma_x (a length in scene units) SPCBPT_REPROJECT_SIGMA_X_FRACTION of the diagonal of
 * the scene's bounding box, as in spcbpt_denoise; a NaN is SPCBPT_ERR_INVALID_ARG.  The defaults (0.5, 0.002, 32) are the triple with
 * the lowest summed rank on the grid {0.1, 0.25, 0.5} x {0.002, 0.005, 0.02} x {16, 32, 64}: RMSE of resolve(1) and resolve(8) against
 * a converged image after orbits of 2 and 8 degrees, Cornell box and bedroom (tools/reproject_grid.py). */
typedef struct spcbpt_reproject_params {
    float sigma_n, sigma_x, max_history;
} spcbpt_reproject_params;
#define SPCBPT_REPROJECT_SIGMA_N 0.5f
#define SPCBPT_REPROJECT_SIGMA_X_FRACTION 0.002f
#define SPCBPT_REPROJECT_MAX_HISTORY 32.0f
int spcbpt_reproject_params_struct_size(void);   /* sizeof(spcbpt_reproject_params) as the library was compiled (spcbpt_abi_struct_sizes keeps its 13 entries) */
/* The three passes are links of the film-merge chain like spcbpt_denoise: they see every merge queued before them, are asynchronous,
 * and their kernel-time spans are "history_capture", "reproject" and "resolve".  All need a film and no deferred frame outstanding;
 * capture and reproject need a feature launch since the last spcbpt_resize, reproject a captured history of the current film size
 * (else SPCBPT_ERR_STATE, with text); frames == 0 is SPCBPT_ERR_INVALID_ARG.  Resolve works without a prior and is then the film
 * itself.  Five planes, 68 B per pixel (H, G, the prior, the resolved image and its RGBA8 frame), are allocated at the first
 * capture; spcbpt_resize and spcbpt_history_reset free them, spcbpt_clear_accum leaves the history alone.
 * The intended sequence: capture at the old camera, spcbpt_set_camera, spcbpt_launch(alg, 0), spcbpt_launch_features(0), reproject,
 * then resolve(1), spcbpt_launch(alg, 1), resolve(2), ...  The features of both views should be those of subframe 0 (centre rays:
 * P is then the first hit exactly); later feature means still work, they only blur P by the jitter.
 * Not covered: sky pixels (a miss has no depth), spcbpt_film_error on the resolved image (it and the moments plane keep describing
 * the film; the variance of the resolved image is spcbpt_read_history_variance's), sharded films, the batched and deferred launch
 * forms, moving geometry.  A reprojected highlight lags for up to max_history frames. */
int spcbpt_history_capture(spcbpt_ctx* ctx, uint32_t frames);
int spcbpt_history_reproject(spcbpt_ctx* ctx, const spcbpt_reproject_params* params);
int spcbpt_history_resolve(spcbpt_ctx* ctx, uint32_t frames);
/* Drops history and prior and frees their planes (waits for the context's streams). */
int spcbpt_history_reset(spcbpt_ctx* ctx);
/* Waits like spcbpt_read_denoised and copies the float4 resolved image, its RGBA8 frame, the prior and H (any pointer may be NULL).
 * SPCBPT_ERR_STATE for a plane that does not exist yet: nothing resolved, no live prior, nothing captured. */
int spcbpt_read_history(spcbpt_ctx* ctx, float* resolved_rgba, uint8_t* resolved_rgba8, float* prior_rgba, float* history_rgbn);
/* The same per-pixel functions on caller buffers on the host; no context and no GPU needed.  Cameras as spcbpt_set_camera takes
 * them, float4-per-pixel planes as the read-backs give them.  Without a scene the default of sigma_x is
 * SPCBPT_REPROJECT_SIGMA_X_FRACTION of sigma_x_default_diag (<= 0: 1).  The inputs are not written.  SPCBPT_ERR_INVALID_ARG for a
 * NULL pointer (the resolve's prior may be NULL: no prior), an empty image, a NaN parameter or frames == 0. */
int spcbpt_history_reproject_host(const float eye[3], const float U[3], const float V[3], const float W[3], const float* normal_depth_rgba,
                                  const float eye_h[3], const float U_h[3], const float V_h[3], const float W_h[3],
                                  const float* history_normal_depth_rgba, const float* history_rgbn, int width, int height,
                                  const spcbpt_reproject_params* params, float sigma_x_default_diag, float* prior_out);
int spcbpt_history_resolve_host(const float* prior_rgba, const float* accum_rgba, uint32_t frames, int64_t n_pixels, float* out_rgba);

/* The variance of what is shown, carried through the history, and the variance-guided denoiser on the resolved image (no reference
 * counterpart), opt-in.  "Variance" is the per-channel variance of the MEAN of a pixel, in a float4 plane (V_r, V_g, V_b, 0) in the
 * film's row order; float32 without contraction throughout.
 * Film variance VA(p), from accum and the moments plane m2n = (M2, n) (a plane that does not exist yet counts as n = 0 everywhere):
 *   n >= 2:  VA_k = max(M2_k, 0) / (n (n - 1))      (the operations of sd_k above before its square root: sqrtf(VA_k) is sd_k bit for bit)
 *   n <  2:  VA_k = accum_k^2                       (unknown variance: as uncertain as its own value, per channel; the one branch, on the integer n)
 * History variance HV(q): the variance of H(q).rgb, taken at capture.
 * Prior variance PV(p): the reprojection's own taps, weights w_q and sum S with HV as the payload,
 *   PV_k = sum_q w_q HV_k(q) / S,      0 wherever R(p) = 0 (a miss, g <= 0, S < 1e-6)
 * -- linear in the variance, not w_q^2: neighbouring history pixels share light sub-paths and the taps of earlier interpolations, so
 * they are not independent and the w^2 rule would understate the variance.  max_history clamps what the prior is worth (m), not how
 * uncertain its value is: PV is not rescaled by it.
 * Resolved variance RV(p), with m = R(p).w and Nf = (float)frames as in the resolve:
 *   RV_k = (m^2 PV_k + Nf^2 VA_k) / (m + Nf)^2;      while no prior is live RV = VA bit for bit (the value, not the formula with m = 0)
 * VA uses the moments plane's own n; `frames` only weights, as in the blend.  Capture: HV becomes the RV of the capture's resolve (a
 * live prior is folded in, so a chain of moves keeps its variance as H keeps its history).
 * The history carries variance exactly while the moments switch (spcbpt_set_film_moments) is on: a capture made then also writes HV,
 * a reproject of a history that has HV also writes PV (one pass, the weights computed once), a resolve made then also writes RV -- a
 * live prior has to have PV for that.  Prior, resolved image and RGBA8 frame are the same bits either way; with the switch off the
 * calls run the kernels they always ran and no variance plane counts as valid.  Three more float4 planes, 48 B per pixel, each
 * allocated by the first call that writes it, freed with the history planes; switching the moments off invalidates them.
 * History denoise: the iterations, guides, step parameters, remodulation and output planes of spcbpt_denoise_variance (read with
 * spcbpt_read_denoised), started from the resolved image (w = (0.3, 0.6, 0.1)):
 *   c_0(p) = resolved(p).rgb / max(albedo(p).rgb, 1e-3)
 *   v_0(p) = (sum_k w_k sqrtf(RV_k(p)) / max(albedo_k(p), 1e-3))^2
 * so a re-used pixel is filtered as narrowly as its history deserves and a disoccluded one as widely as its single sample needs.  On
 * a film whose pixels all have n >= 2, with no prior live, the output is spcbpt_denoise_variance's bit for bit.  sigma_c is read as
 * sigma_v; defaults and argument checks are spcbpt_denoise_variance's.  A link of the film-merge chain, asynchronous; the kernel-time
 * span is "history_denoise".  Needs a feature launch since the last spcbpt_resize, a resolve that produced RV since the last resize
 * or reset, and no deferred frame outstanding (else SPCBPT_ERR_STATE, with text).  Writes the denoiser's planes only.
 * Not covered: sky pixels, spcbpt_film_error on the resolved image, sharded films and the N-GPU host, the batched and deferred
 * launch forms, a specular / diffuse split, temporal accumulation of per-sample moments (SVGF's way of steadying a 2-frame variance). */
int spcbpt_history_denoise(spcbpt_ctx* ctx, const spcbpt_denoise_params* params);
/* Waits like spcbpt_read_history and copies RV, PV and HV (any pointer may be NULL).  SPCBPT_ERR_STATE for a plane that is not valid:
 * nothing resolved / no live prior / nothing captured, or the moments were off when it was. */
int spcbpt_read_history_variance(spcbpt_ctx* ctx, float* resolved_var, float* prior_var, float* history_var);
/* The same per-pixel functions on caller buffers on the host; no context and no GPU needed.  The reprojection takes
 * spcbpt_history_reproject_host's arguments plus HV and the plane for PV (prior_out is that call's, bit for bit); the resolve's
 * prior_rgba and prior_var are both NULL (no prior) or both given; the denoise takes the resolved image and RV with the feature
 * planes as spcbpt_denoise_variance_host does.  SPCBPT_ERR_INVALID_ARG as for their siblings. */
int spcbpt_history_reproject_var_host(const float eye[3], const float U[3], const float V[3], const float W[3], const float* normal_depth_rgba,
                                      const float eye_h[3], const float U_h[3], const float V_h[3], const float W_h[3],
                                      const float* history_normal_depth_rgba, const float* history_rgbn, const float* history_var,
                                      int width, int height, const spcbpt_reproject_params* params, float sigma_x_default_diag,
                                      float* prior_out, float* prior_var_out);
int spcbpt_history_resolve_var_host(const float* prior_rgba, const float* prior_var, const float* accum_rgba, const float* m2n, uint32_t frames,
                                    int64_t n_pixels, float* out_rgba, float* out_var);
int spcbpt_history_denoise_host(const float* resolved_rgba, const float* resolved_var, const float* albedo_rgba, const float* normal_depth_rgba,
                                const float eye[3], const float U[3], const float V[3], const float W[3],
                                int width, int height, const spcbpt_denoise_params* params, float* out_rgba);

int spcbpt_get_counters(spcbpt_ctx* ctx, spcbpt_counters* out);
int spcbpt_reset_counters(spcbpt_ctx* ctx);
/* Developer aid (no reference counterpart): wave-clock totals the counting build of the "SPCBPT_eye" megakernel spent in
 * its phases since the last reset: [0] regeneration, [1] closest-hit traversal, [2] vertex + resampling, [3] pooled shadow
 * traversal, [4] connection + film (only ratios are meaningful); [5..8] lane utilisation of the traversal loops of all
 * kernels: node-loop slots (64 x wave iterations) and lanes, triangle-loop slots and lanes; [9] lane-clocks of the two-stage
 * resampling (part of [2], summed over the lanes that sample); [10..13] 100 MHz wall clock of the megakernel's waves: earliest
 * start, latest end, sum of ends, number of waves (how long the last waves run alone); [14..16] the tail of the pooled traversal
 * pass, i.e. its node steps after the wave's ray pool ran dry: slots (64 x iterations), lanes still on a closest-hit ray, lanes on
 * a shadow ray; [17..18] the connection evaluations of the connect phase: slots (64 x rounds of its job loop) and jobs. */
int spcbpt_debug_phase_clocks(spcbpt_ctx* ctx, uint64_t out[19]);
/* Hash of the sources this library was built from (csrc/source_hash.py); the Python mirror refuses a stale library. */
const char* spcbpt_build_source_hash(void);
/* The FP32 arithmetic of this library's device code: "ieee" for libspcbpt_hip.so (correctly rounded division and square root,
 * no contraction -- the oracle's operations; what every function-level parity test and the film hashes assume), "approx" for the
 * opt-in libspcbpt_hip_fast.so (hardware reciprocal / square root, as the reference's own `--use_fast_math` build,
 * src/CMakeLists.txt:214; image-level bars only: tests/test_gpu_fast_build.py). */
const char* spcbpt_build_arithmetic(void);
/* sizeof of the structs of this header as the library was COMPILED, in declaration order: material, texture, quad_light,
 * scene_desc, tree_node, light_trace_params, light_vertex, subspace, counters, unit_eye_vertex, pretrace_path,
 * pretrace_node, viewer_state.  A binding in another language (ctypes / cgo / JNI) checks its mirrors against these instead of
 * against literals (tests/test_abi.py).  Returns the number of structs (13) and writes min(capacity, 13) sizes. */
int spcbpt_abi_struct_sizes(int32_t* sizes, int capacity);
/* Developer probe of the HBM part of the traversal stack.  The per-lane stack holds SPC_STACK_LDS (16) entries in LDS; deeper
 * entries go to a per-thread spill area of 3 * bvh_depth - 16 words, which cannot overflow.  _arm fills every area allocated
 * so far with a word no stack entry can hold, _count returns how many words kernels have overwritten since (tests prove the
 * spill path ran) and the entries per thread.  Should a kernel ever drop an entry (SPCBPT_DEBUG_SPILL_ENTRIES=n in the
 * environment at spcbpt_create caps the area, for tests), spcbpt_sync / spcbpt_read_* / spcbpt_trace_* return
 * SPCBPT_ERR_STATE once and name the count: the reference's optixTrace has no such failure mode, a lost subtree is never silent. */
int spcbpt_debug_spill_arm(spcbpt_ctx* ctx);
int spcbpt_debug_spill_count(spcbpt_ctx* ctx, uint64_t* words_written, int* entries_per_thread);

/* "Plain BDPT", the comparator BASELINE config 5 names: with mode = SPCBPT_SAMPLER_UNIFORM the "SPCBPT_eye" launch draws each of
 * its CONNECTION_N light vertices with SubspaceSampler_device::uniformSample (cuProg.h:283-289: uniform over jump_buffer, pmf
 * 1 / vertex_count, one random number) instead of sampleFirstStage + sampleSecondStage; everything else -- shadow ray,
 * connectVertex_SPCBPT, recursive MIS weights (a partition of unity over strategies whatever the sampler) -- is unchanged, so
 * the estimator stays unbiased.  The reference defines uniformSample and never calls it.  Default SPCBPT_SAMPLER_SUBSPACE. */
enum { SPCBPT_SAMPLER_SUBSPACE = 0, SPCBPT_SAMPLER_UNIFORM = 1 };
int spcbpt_set_connection_sampler(spcbpt_ctx* ctx, int mode);

/* Per-function device harness (tests/test_gpu_units.py): evaluates ONE device function of the hot path on n caller-supplied
 * records (one lane each) with the context's scene, subspace tuple and -- for STAGE2 / UNIFORM -- the sampler of the last
 * spcbpt_build_sampler.  Records are arrays of 32-bit words (floats by bit pattern), `in_words` / `out_words` per record:
 *   SPCBPT_UNIT_BSDF     in 24: material(base3, metallic, roughness, specular, specular_tint, subsurface, sheen, sheen_tint, clearcoat,
 *                        clearcoat_gloss) N3 V3 L3 seed pad2        out 12: Sample(N,V;seed)3, seed', Eval(N,V,L)3, Pdf(N,V,L), Eval(N,V,Ls)3, Pdf(N,V,Ls)
 *   SPCBPT_UNIT_TREE     in 10: tree(0 eye, 1 light) position3 normal3 direction3                      out 1: label
 *   SPCBPT_UNIT_STAGE1   in 2: eye subspace, seed        out 6: l, pmf, seed' as the kernels sample (guide table + window) ; l, pmf, seed' by binary_sample
 *   SPCBPT_UNIT_BSEARCH  in 3: offset, size, seed (CMF = aux + offset)                                  out 3: bin, pmf, seed'
 *   SPCBPT_UNIT_STAGE2   in 2: light subspace, seed                                                     out 5: size, bin (-1: empty), LVC slot, pmf, seed'
 *   SPCBPT_UNIT_UNIFORM  in 1: seed                                                                     out 3: LVC slot, pmf, seed'
 *   SPCBPT_UNIT_CONNECT  in 52: eye vertex (spcbpt_unit_eye_vertex, 25) light vertex (spcbpt_light_vertex, 24) form, lsub, pad
 *                        out 4: connectVertex_SPCBPT rgb, RMIS weight; with out_words >= 5 also word 4: 1 where null_connection /
 *                        null_connection_direction call the pair null -- the test by which the eye megakernel skips a connection
 *                        and its shadow ray -- else 0
 *   SPCBPT_UNIT_EYE_STEP in 36: last eye vertex (25) NextVertex.flux3 NextVertex.singlePdf seed ray direction3 flags(bit 0: d11) form, lsub
 *                        out 40: kind (0 miss, 1 surface vertex, 2 emitter front, 3 emitter back), new vertex (25), next direction3,
 *                        NextVertex.flux3, NextVertex.singlePdf, seed', done, emitter radiance3 (lightStraghtHit), t_hit, and the new
 *                        vertex's own light-tree label `lsub` as the cached forms derive it (0 in the reference form and at depth 1).
 *                        For an emitter hit the vertex words hold the LIGHT's record at the hit point, as a light sample of that
 *                        point would: position, normal, pdf = single_pdf, material_id = light id, subspace_id = its patch label.
 *   SPCBPT_UNIT_SKY_MISS in 32: last eye vertex (25) NextVertex.flux3 NextVertex.singlePdf escape direction3 (towards the sky)
 *                        out 6: contribution rgb of the eye path that sees the sky (SPCBPT_ENV_EYE_SEES_SKY), its RMIS weight
 *                        (1 / RMIS_pointer), the sky's subspace label, pad.  Needs an environment map (else SPCBPT_ERR_STATE).
 *                        With in_words >= 34, words 32 / 33 are form / lsub.
 *   SPCBPT_UNIT_STAGE2_GUIDED in 6: CONNECTION_N light subspaces, CONNECTION_N random numbers (float bits, in [0, 1))
 *                        out 12: per connection size, bin (-1: empty subspace, skipped), place in the sorted cache (jump_bias + bin), pmf
 *                        -- the second-stage draw AS THE EYE MEGAKERNEL RUNS IT (guide table + aligned windows of eight CMF entries,
 *                        csrc/second_stage_guided.inc.h, the text both compile); STAGE2 above is the reference's bisection.
 *   SPCBPT_UNIT_SORTED   in 1: place i in the sorted cache (i >= vertex count: zeros)   out 24: the 96 bytes of record i
 *                        (spcbpt_light_vertex), = the cache's record jump[i]
 *   SPCBPT_UNIT_ENV      in 4: direction3 (as given: not normalised), seed
 *                        out 24: dir2uv(direction) u, v; env_color3, env_pdf (per solid angle, not yet divided by the light count),
 *                        env_label of the direction; env_sample(seed)3, seed'; then everything env_light_sample returns for the
 *                        SAME starting seed: position3, emission3, normal3, pdf (divided by the light count), subspace, dir_pos_pdf, seed'
 *   SPCBPT_UNIT_ENV_TABLE in 1: texel index i (>= width * height: SPCBPT_ERR_INVALID_ARG)
 *                        out 5: the sampling CMF's entry i (over the raster as read), the four floats of texel i of the row-flipped texture
 *   SPCBPT_UNIT_TEX      in 3: texture number as spcbpt_material::albedo_tex counts it (1 .. n_textures, else SPCBPT_ERR_INVALID_ARG), u, v
 *                        out 6: tex_fetch_rgb3 (bilinear, wrap), the linearised colour3 a hit stores (powf(., 2.2f))
 * STAGE2, UNIFORM, STAGE2_GUIDED and SORTED need a built sampler, ENV and ENV_TABLE an environment map (else SPCBPT_ERR_STATE);
 * BSDF, BSEARCH, ENV, ENV_TABLE and TEX run without a subspace tuple.
 * The ray of EYE_STEP starts at the last vertex's position.  Host pointers; returns after the kernel has run.
 * `form` (CONNECT, EYE_STEP, SKY_MISS) selects the instantiation of connect_vertices / eye_surface_hit / eye_emitter_hit /
 * eye_sky_miss that evaluates the record -- the same text, three programs:
 *   SPCBPT_UNIT_FORM_REFERENCE (0)     CACHE = false, ENV = true: every label by a descent of its tree, as the reference does and
 *                                      as the counting kernels run; a record with zero pad words means what it always meant
 *   SPCBPT_UNIT_FORM_CACHED (1)        CACHE = true, ENV = true: what the timed kernels run on a `general` scene (environment map,
 *                                      `brdf`-flagged material, mesh light).  The eye vertex's light-tree label is the input word
 *                                      `lsub`, the light vertex's eye-tree label the low 16 bits of its `pad` minus 1 (0: an imported
 *                                      cache without labels, the descent happens); EYE_STEP labels the new vertex under both trees
 *   SPCBPT_UNIT_FORM_CACHED_PLAIN (2)  CACHE = true, ENV = false: the timed kernels of a plain scene -- no direction flags, no
 *                                      brdf division, no mesh-light branch.  SKY_MISS has no such form (SPCBPT_ERR_INVALID_ARG).
 * What no launcher would pick is refused with SPCBPT_ERR_STATE: a cached form while the classifier trees hold direction nodes
 * (cached labels do not depend on the direction), CACHED_PLAIN on a `general` scene.  `lsub` and the cached `pad` label index the
 * Gamma table unchecked, as in the timed kernels: the caller keeps them in [0, SPCBPT_NUM_SUBSPACE) (the host refuses others). */
enum { SPCBPT_UNIT_FORM_REFERENCE = 0, SPCBPT_UNIT_FORM_CACHED = 1, SPCBPT_UNIT_FORM_CACHED_PLAIN = 2 };
typedef struct spcbpt_unit_eye_vertex {   /* the BDPTVertex fields an eye sub-path vertex carries (BDPTVertex.h:9-70) */
    float position[3], normal[3], flux[3], color[3], last_position[3], rmis3[3];
    float pdf, single_pdf, last_normal_projection;
    int32_t material_id, subspace_id, depth, last_zone_id;
} spcbpt_unit_eye_vertex;
enum spcbpt_unit_op { SPCBPT_UNIT_BSDF = 0, SPCBPT_UNIT_TREE = 1, SPCBPT_UNIT_STAGE1 = 2, SPCBPT_UNIT_BSEARCH = 3, SPCBPT_UNIT_STAGE2 = 4,
                      SPCBPT_UNIT_UNIFORM = 5, SPCBPT_UNIT_CONNECT = 6, SPCBPT_UNIT_EYE_STEP = 7, SPCBPT_UNIT_SKY_MISS = 8,
                      SPCBPT_UNIT_STAGE2_GUIDED = 9, SPCBPT_UNIT_SORTED = 10, SPCBPT_UNIT_ENV = 11, SPCBPT_UNIT_ENV_TABLE = 12,
                      SPCBPT_UNIT_TEX = 13 };
int spcbpt_debug_unit(spcbpt_ctx* ctx, int op, const uint32_t* in, int in_words, uint32_t* out, int out_words, int n,
                      const float* aux, int aux_floats);

/* Developer A/B of two traversal schedules on the SAME rays (round 4, csrc/quad_trace.hip): mode 0 = one lane per ray (the loop
 * of the render kernels), mode 1 = four lanes per ray (one coalesced 64-B node fetch per visit, one child box / one leaf
 * triangle per lane), modes 2 / 3 = the same with 2 / 4 rays per quad in flight; all persistent and pool-fed.  rays: n x {origin3, tmin, direction3, tmax}; any != 0: terminate on first hit
 * (visibilityTest semantics, out_visible) else nearest hit with emitter culling (out_t / out_tri / out_uv; the unused outputs may be
 * NULL).  The launch is repeated `repeat` times on device-resident rays; *avg_ms is the HIP-event mean of one launch.  stats (may be
 * NULL): [0] node visits, [1] leaf visits, [2] triangle tests, [3] lane slots (64 x wave iterations), [4] lanes holding a ray in them,
 * from one more, counting launch.  Mode 1 needs 3 x BVH depth <= 64, modes 2 / 3 <= 48 (their per-ray LDS stacks). */
int spcbpt_debug_trace_bench(spcbpt_ctx* ctx, const float* rays, int n, int mode, int any, int repeat, float* out_t, int32_t* out_tri,
                             float* out_uv, int32_t* out_visible, double* avg_ms, uint64_t stats[5]);
/* Per-ray entry point of the POOLED traversal pass of the eye megakernel (csrc/pool_trace.hip; tests/test_gpu_ray_verdict.py): one pass
 * of trace_pool over n lanes, lane i being lane i % 64 of wave i / 64, in the megakernel's block, stack and hot-node table.
 *   own_rays   n x {origin3, -, direction3, -}: the lane's own closest-hit ray, traced over (SPCBPT_SCENE_EPSILON, 1e16) where own_mask[i] != 0
 *   shadow_org n x {position3, -}: the lane's eye vertex, the origin of its shadow rays
 *   shadow_rays n x SPCBPT_CONNECTION_N x {direction3, length}: length < 0 = empty slot; a ray is traced over
 *              (SPCBPT_SCENE_EPSILON, length - SPCBPT_SCENE_EPSILON).  In/out: on return the length of an OCCLUDED ray is -1.
 *   out_t / out_tri / out_uv: n hit records (tri -1: a miss, or no own ray).
 * Host pointers; n need not be a multiple of 64 (the last wave's other lanes hold nothing).  Returns after the kernel has run. */
int spcbpt_debug_trace_pool(spcbpt_ctx* ctx, int n, const float* own_rays, const int32_t* own_mask, const float* shadow_org, float* shadow_rays,
                            float* out_t, int32_t* out_tri, float* out_uv);
/* Event counting in the kernels (off for timed runs).  1: the counting instantiations evaluate in the REFERENCE's order and charge
 * its events (two relabels per connection and one per RMIS update, a ten-probe bisection per first sampling stage): the contract's
 * byte table of SURVEY.md 8(d).  2: the instantiations the timed runs use, with counters -- the events that really execute (labels
 * cached per vertex; one guide entry + eight CMF values per window of either resampling stage, one Gamma / Q value per
 * evaluation): what the roofline fraction is computed from. */
int spcbpt_enable_counters(spcbpt_ctx* ctx, int enabled);

/* Streams.  A context owns two non-blocking HIP streams: the one returned here (hipStream_t as void*) carries "light trace",
 * the sampler build, LVC import/export copies and the preprocessing; render launches ("pt", "SPCBPT_eye") go to a second one,
 * ordered against the first with events, so that the next frame's light pass can run while an eye kernel drains.
 * spcbpt_sync waits for both (the CUDA_SYNC_CHECK() of the reference's loop); spcbpt_sync_light waits only for the light /
 * sampler stream -- what a multi-GPU host needs before it all-gathers the LVC shard (no reference counterpart). */
int spcbpt_stream(spcbpt_ctx* ctx, void** stream);
int spcbpt_sync(spcbpt_ctx* ctx);
int spcbpt_sync_light(spcbpt_ctx* ctx);
/* A frame ahead in the interactive loop (no reference counterpart; optixPathTracer.cpp:791-822 renders and displays strictly in
 * turn).  spcbpt_launch_deferred is spcbpt_launch("pt" | "SPCBPT_eye", ...) WITHOUT the film merge: the kernel renders into a buffer
 * of its own, accum / frame are untouched.  spcbpt_merge_deferred(ctx, 1) queues that merge -- from then on the frame is exactly
 * what spcbpt_launch would have produced -- and (ctx, 0) drops the frame (the camera moved: its samples belong to no image).  One
 * frame may be outstanding; until it is merged or dropped every other render launch (spcbpt_launch "pt" / "SPCBPT_eye" /
 * "SPCBPT_no_rmis", spcbpt_launch_deferred, spcbpt_launch_eye_batch), spcbpt_clear_accum and spcbpt_set_light_ahead return
 * SPCBPT_ERR_STATE -- the film would otherwise take frames out of order (spcbpt_resize drops it).
 * spcbpt_sync_film makes the host wait for the LAST QUEUED film merge only: the frame to display is complete, work queued behind it
 * (the next frame's light pass, sampler build, deferred eye launch) keeps running.  csrc/viewer.cpp builds its default loop on
 * these: frame f+1 is traced while frame f is shown, and every displayed frame is the reference loop's frame. */
int spcbpt_launch_deferred(spcbpt_ctx* ctx, const char* alg, uint32_t subframe_index, int row_begin, int row_end, int row_step);
int spcbpt_merge_deferred(spcbpt_ctx* ctx, int keep);
int spcbpt_sync_film(spcbpt_ctx* ctx);
/* Batched eye launch (no reference counterpart): renders the samplers of the last n_frames spcbpt_build_sampler calls -- one
 * frame each, oldest first, subframe index subframes[k] -- with ONE persistent kernel whose tile queue spans the frames, and
 * merges them into the film in that order.  The result is that of n_frames spcbpt_launch("SPCBPT_eye") calls; the point is the
 * drain phase of the megakernel, which is paid once per launch: a rank's eighth of a sharded frame is about one 8x8 tile per
 * resident wave, i.e. nothing but drain.  n_frames <= 32 and <= the number of samplers built since and still intact
 * (SPCBPT_ERR_STATE otherwise).  SPCBPT_EYE_BATCH = F in the environment at spcbpt_create sizes the ring of sampler buffer
 * sets for batches of F, so that batches in flight, light passes ahead and builds never wait for a set. */
int spcbpt_launch_eye_batch(spcbpt_ctx* ctx, int n_frames, const uint32_t* subframes, int row_begin, int row_end, int row_step);
/* The same launch -- arguments, preconditions, eye kernel -- whose merge also keeps the film's second moment (spcbpt_set_film_moments)
 * and fills its buckets (spcbpt_set_film_buckets), whichever are on: one pass in which every pixel takes the frames in order and does,
 * per frame, exactly what the moments update, the bucket update and the merge of spcbpt_launch do.  accum, frame, the moment plane and
 * the bucket planes are bit for bit those of n_frames spcbpt_launch("SPCBPT_eye") calls, so spcbpt_film_error, spcbpt_denoise_variance,
 * spcbpt_adaptive_begin and spcbpt_robust_resolve see the film they would have seen.  With both switches off the call is
 * spcbpt_launch_eye_batch.  SPCBPT_ERR_STATE with a text that names the reason while adaptive sampling is active, a deferred frame is
 * outstanding, a lens is set, event counters are on or the classifier trees have direction nodes; SPCBPT_ERR_INVALID_ARG for n_frames
 * outside 1 .. 32.  The kernel-time span of the merge is "film_merge_stats". */
int spcbpt_launch_eye_batch_film(spcbpt_ctx* ctx, int n_frames, const uint32_t* subframes, int row_begin, int row_end, int row_step);
/* That merge of n_pixels pixels on the host: the per-pixel function the kernel runs (float32, no contraction).  samples is
 * [n][n_pixels] float4, the frames' samples in batch order with subframes[k] their subframe indices; accum_inout [n_pixels] float4 (its
 * alpha becomes 1, as the film's); m2n_inout_or_null [n_pixels] float4, NULL = no moments; planes_inout_or_null [buckets][n_pixels]
 * float4 with buckets = 3 .. 32, or buckets = 0 (the pointer is then ignored).  All updated in place.  No context and no GPU needed.
 * SPCBPT_ERR_INVALID_ARG for a NULL samples / subframes / accum, n outside 1 .. 32, n_pixels outside 1 .. 2^28, buckets not 0 or
 * 3 .. 32, or buckets without planes. */
int spcbpt_film_merge_batch_host(const float* samples, const uint32_t* subframes, int n, int64_t n_pixels, int buckets,
                                 float* accum_inout, float* m2n_inout_or_null, float* planes_inout_or_null);
/* Batched light pass (no reference counterpart; needs spcbpt_set_light_ahead on): the "light trace" launches of launch frames
 * first_frame .. first_frame + n_frames - 1 as ONE persistent kernel whose core queue spans the frames.  Every pass lands in its own
 * buffer set and queues up exactly as n_frames spcbpt_launch("light trace", first_frame + k) calls would have left them -- the caches
 * are bit-identical to those -- so the host goes on with n_frames x (export / import, spcbpt_build_sampler) and one
 * spcbpt_launch_eye_batch.  The point is again the dependent chain: a rank of an 8-GPU job traces 1/8 of the cores per frame, each
 * pass still takes the ~1.2 ms of its longest path, and beside the eye grid they run one after the other; in one queue they cost
 * about one full-size pass.  n_frames <= 32 (SPCBPT_ERR_INVALID_ARG), SPCBPT_ERR_STATE without light-ahead mode. */
int spcbpt_launch_light_batch(spcbpt_ctx* ctx, uint32_t first_frame, int n_frames);
/* Batched sampler build (no reference counterpart): n_builds spcbpt_build_sampler calls -- the n_builds OLDEST queued light
 * passes -- with the kernels of ONE build (the frame in the grid's second dimension).  Same tables, same state afterwards; what
 * goes is the chain of 4 x n_builds small dependent launches in front of a batched eye launch that cannot start before the last
 * of them (0.12 ms per build on the bench scene).  With SPCBPT_SAMPLER_BUILD=hipcub, or for a cache whose counts the host has to
 * read back first, the call is n_builds times spcbpt_build_sampler -- and also when the device cannot hold the batch's scratch
 * (n_builds x the largest item bound among the builds x 16 B; it only grows, spcbpt_lvc_set_capacity and leaving light-ahead mode
 * free it).  1 <= n_builds <= 32 (SPCBPT_ERR_INVALID_ARG). */
int spcbpt_build_sampler_batch(spcbpt_ctx* ctx, int n_builds);
/* Test hook: bytes and frames of that scratch, and how many batches fell back to single builds for want of it
 * (SPCBPT_DEBUG_BATCH_SCRATCH_LIMIT=<bytes> in the environment makes larger requests fail). */
int spcbpt_debug_batch_scratch(spcbpt_ctx* ctx, int64_t* bytes, int* frames, int* fallbacks);
/* Test hook: host copies of the tables the eye kernel samples through (no reference counterpart; csrc/layout.h KParams::guide,
 * cmf_guide1, gamma_q).  guide2: one entry per light vertex of the last sampler build, in the order of spcbpt_sampler_read's cmfs
 * (capacity2 entries at least the vertex count, else SPCBPT_ERR_CAPACITY); guide1: 1000 x 1024 entries; gamma_q: 1000 x 1000.
 * Any of the three may be NULL. */
int spcbpt_debug_read_sampling_tables(spcbpt_ctx* ctx, uint32_t* guide2, int capacity2, uint16_t* guide1, float* gamma_q);

/* Light passes running ahead (multi-GPU host loops; no reference counterpart).  The light pass is a ~1 ms dependent chain
 * however few paths a rank traces, and the LVC exchange makes the host wait for it; with on != 0 the host may launch frame
 * f + 1's "light trace" BEFORE it exchanges and builds frame f's: every light pass queues its buffer set, and
 * spcbpt_lvc_export / spcbpt_lvc_import / spcbpt_sync_light / spcbpt_build_sampler address the OLDEST queued pass (sync_light
 * then waits for that pass only, not for the stream).  Off (default): they address the latest light pass.  Either way a "light
 * trace" launch invalidates the sampler for eye launches (SPCBPT_ERR_STATE until the next spcbpt_build_sampler), as the reference's
 * loop implies.  Switching waits for the context's streams, clears the queue of unbuilt passes and, when switched off, frees the
 * batched build's scratch. */
int spcbpt_set_light_ahead(spcbpt_ctx* ctx, int on);
/* What the context holds of a loop that runs ahead: light-ahead mode, the number of light passes launched but not built yet, whether
 * the tables of the LAST sampler build are still intact (no later pass, import or re-allocation took their buffer set), whether a
 * deferred frame is outstanding.  Any pointer may be NULL. */
int spcbpt_get_pipeline_state(spcbpt_ctx* ctx, int* light_ahead, int* pending_passes, int* sampler_intact, int* deferred_outstanding);
/* Render once more from the sampler built last although a later "light trace" has been launched since (with passes ahead it went to
 * another buffer set): the interactive loop's re-render of a frame whose speculative launch was dropped.  SPCBPT_ERR_STATE if the
 * tables are gone. */
int spcbpt_reuse_sampler(spcbpt_ctx* ctx);
/* spcbpt_lvc_import(..., is_device = 1) reads its source asynchronously (on the light stream, possibly behind light passes launched
 * ahead).  A host that alternates TWO staging buffers calls this before it overwrites one of them: it returns when the import
 * before the previous one -- the last reader of that buffer -- has copied. */
int spcbpt_lvc_import_wait(spcbpt_ctx* ctx);

/* Kernel timing measured with HIP events on the context's stream: average
 * milliseconds per launch of `name` since the last reset, and launch count.  (The film merge behind a render launch is the span
 * "film_merge", the moments update in front of it "moments", the bucket update "buckets"; the display pass is "display_hist" and
 * "display", the bloom stage "bloom", the local tone stage "local_tone".) */
int spcbpt_kernel_time(spcbpt_ctx* ctx, const char* name, double* avg_ms, int* launches);
int spcbpt_reset_kernel_time(spcbpt_ctx* ctx);
int spcbpt_enable_kernel_timing(spcbpt_ctx* ctx, int enabled);

/* Standalone traversal entry points (parity tests of the software LBVH
 * against the oracle's BVH; they are the building block optixTrace is replaced
 * by: cuProg.h:384-461 closest hit, 463-487 visibilityTest).
 * rays: n * 8 floats (origin xyz, tmin, direction xyz, tmax).
 * closest: out_t[n], out_tri[n] (-1 = miss), out_uv[2n]; cull_emitter_backfaces
 * as OPTIX_RAY_FLAG_CULL_BACK_FACING_TRIANGLES acts on the single-sided quads.
 * any: out_visible[n] = 1 when nothing is hit in (tmin, tmax). */
int spcbpt_trace_closest(spcbpt_ctx* ctx, const float* rays, int n,
                         float* out_t, int32_t* out_tri, float* out_uv);
int spcbpt_trace_any(spcbpt_ctx* ctx, const float* rays, int n, int32_t* out_visible);

/* Training records of the "pretrace" pass: values of TrainData::pathInfo_sample and TrainData::pathInfo_node
 * (optixPathTracer.h:325-383).  begin_ind/end_ind index the node array; label_A holds the eye depth until the trees
 * exist (node_label, device_thrust.cu:554-573); label_B is pre-filled for emitter vertices only. */
typedef struct spcbpt_pretrace_path {
    float contri[3];
    float sample_pdf;
    float fix_pdf;
    int32_t begin_ind;
    int32_t end_ind;
    int32_t choice_id;
    int32_t pixel_id[2];
    int32_t valid;
    int32_t pad;
} spcbpt_pretrace_path; /* 48 bytes */

typedef struct spcbpt_pretrace_node {
    float a_position[3];
    float b_position[3];
    float a_dir[3];
    float b_dir[3];
    float a_normal[3];
    float b_normal[3];
    float peak_pdf;
    int32_t path_id;
    int32_t label_a;
    int32_t label_b;
    int32_t valid;
    int32_t light_source;
} spcbpt_pretrace_node; /* 96 bytes */

/* Replaces preTracer_params_setup (optixPathTracer.cpp:479-490): threads per "pretrace" launch (reference 10000) and
 * node slots per thread (reference PRETRACE_CONN_PADDING = 10, the maximum). */
int spcbpt_set_pretrace(spcbpt_ctx* ctx, int num_core, int padding);

/* The training set accumulated by "pretrace" launches (= neat_paths / neat_conns after valid_sample_gather,
 * device_thrust.cu:457-493): counts, host copies, replacement (tests inject the oracle's records), reset. */
int spcbpt_train_records_count(spcbpt_ctx* ctx, int* n_paths, int* n_nodes);
int spcbpt_train_records_read(spcbpt_ctx* ctx, spcbpt_pretrace_path* paths, int cap_paths,
                              spcbpt_pretrace_node* nodes, int cap_nodes);
int spcbpt_train_records_import(spcbpt_ctx* ctx, const spcbpt_pretrace_path* paths, int n_paths,
                                const spcbpt_pretrace_node* nodes, int n_nodes);
int spcbpt_train_records_clear(spcbpt_ctx* ctx);

/* Host-owned preprocessing = preprocessing() (optixPathTracer.cpp:552-608):
 * pretrace -> reweight -> subspace trees -> Q -> labels -> Gamma_0 -> Adam
 * training -> CMF Gamma.  Installs the result with spcbpt_set_subspace.
 * target_paths / target_q_paths are the reference's 2,000,000 each; smaller
 * values give a coarser but still valid tuple. */
int spcbpt_preprocess(spcbpt_ctx* ctx, int target_paths, int target_q_paths, int train);
/* The stages of spcbpt_preprocess one by one, on the records currently held (tests compare each with the oracle):
 * stage 1 = sample_reweight + both subspace trees, 2 = Q from light passes (needs target_q_paths), 3 = node labels +
 * outlier clean + Gamma_0, 4 = Adam training, 5 = CMF Gamma + install.  image_width is the 10x10-pixel tile pitch of
 * sample_reweight (the reference hard-codes 1920). */
int spcbpt_preprocess_stage(spcbpt_ctx* ctx, int stage, int arg);
/* Intermediate results for tests / checkpoints: Gamma before the CMF transform (row-major 1000x1000). */
int spcbpt_get_gamma(spcbpt_ctx* ctx, float* gamma);

/* Checkpoint files of the subspace tuple in the reference's own text formats (row f4): tree_eye.txt, tree_light.txt
 * (classTree::tree_load, decisionTree/classTree_host.h:15-59), Q.txt (MyThrustOp::load_Q_file,
 * cuda_thrust/device_thrust.cu:3389-3404) and E.txt = Gamma before the CMF transform (load_Gamma_file, 3347-3380).  The
 * reference has only the readers, with their call sites commented out (optixPathTracer.cpp:573-581, 597, 603); the
 * writers emit what those readers parse.  The first three need neither a context nor a GPU.
 *   spcbpt_checkpoint_read: `gamma` (NUM_SUBSPACE^2) is in/out.  As in load_Gamma_file, the columns of the emitter
 *   subspaces (light id >= NUM_SUBSPACE - NUM_SUBSPACE_LIGHTSOURCE) keep the caller's current values when
 *   have_current_gamma != 0; with 0 every entry comes from the file.
 *   spcbpt_gamma_to_cmf = MyThrustOp::Gamma2CMFGamma (3406-3433).
 *   spcbpt_checkpoint_save writes the installed trees and Q plus the Gamma of the last preprocessing run (SPCBPT_ERR_STATE
 *   if the context never preprocessed: a CMF Gamma handed to spcbpt_set_subspace cannot be inverted exactly).
 *   spcbpt_checkpoint_load reads the four files, applies Gamma2CMFGamma and installs the tuple (spcbpt_set_subspace). */
int spcbpt_checkpoint_write(const char* dir, const spcbpt_tree_node* eye_tree, int n_eye,
                            const spcbpt_tree_node* light_tree, int n_light, const float* q, const float* gamma);
int spcbpt_checkpoint_read(const char* dir, spcbpt_tree_node* eye_tree, int* n_eye, int cap_eye,
                           spcbpt_tree_node* light_tree, int* n_light, int cap_light, float* q, float* gamma,
                           int have_current_gamma);
int spcbpt_gamma_to_cmf(const float* gamma, float* cmf_gamma);
int spcbpt_checkpoint_save(spcbpt_ctx* ctx, const char* dir);
int spcbpt_checkpoint_load(spcbpt_ctx* ctx, const char* dir);

/* Texture file -> RGBA8 as the reference's stbi_load(path, &w, &h, &c, STBI_rgb_alpha) delivers it
 * (OptiXPathTracer/scene_shift.cpp:35-40): baseline / progressive JPEG, PNG, binary PPM, chosen by content.  Two-call
 * protocol: rgba == NULL returns the size only.  The scene loaders use the same decoder.  Needs no context, no GPU. */
int spcbpt_image_load(const char* path, int* width, int* height, uint8_t* rgba, size_t capacity_bytes);

/* Row f3 -- the interactive loop without a window: the state machine of optixPathTracer.cpp (GLFW callbacks 121-241,
 * updateState / handleCameraUpdate / handleResize 333-379, initCameraState 661-670, one pass of the render loop 791-822)
 * over sutil::Trackball and sutil::Camera.  A front end forwards its window events one to one (the arguments are GLFW's:
 * button 0 left / 1 right, action 1 press / 2 repeat / 0 release, key codes ESCAPE 256, SPACE 32, C 67, P 80, W 87) and
 * calls spcbpt_viewer_frame once per displayed subframe; tools/spcbpt_viewer.cpp replays an event script.  `ctx` may be
 * null: the state machine then runs without launching (tests).  Left drag orbits the eye (LookAtFixed), right drag turns
 * the view (EyeFixed), the wheel zooms, SPACE switches pt <-> SPCBPT_eye and restarts the accumulation, P restarts it on
 * every frame, W walks forward by 0.5 / render_fps, ESCAPE sets should_close. */
typedef struct spcbpt_viewer spcbpt_viewer;
typedef struct spcbpt_viewer_state {
    float eye[3], lookat[3], up[3];
    float U[3], V[3], W[3];          /* Camera::UVWFrame at the current window aspect */
    float fov_y, aspect;
    int32_t width, height;
    uint32_t subframe_index;         /* index the NEXT frame will render (0 after a camera / size / algorithm change) */
    int32_t alg_id;                  /* 0 "pt", 1 "SPCBPT_eye" (render_alg, optixPathTracer.cpp:91) */
    int32_t should_close, one_frame_render_only, camera_changed;
    float render_fps;
} spcbpt_viewer_state;
int spcbpt_viewer_create(spcbpt_ctx* ctx, const float eye[3], const float lookat[3], const float up[3], float fov_y,
                         int width, int height, spcbpt_viewer** out);
/* Either order of tear-down is safe (round 6): spcbpt_destroy(ctx) tells the context's live viewers, which go on as state machines
 * without a context (events and frames still advance their state, nothing is launched); destroying the viewer first hands the
 * context back as spcbpt_viewer_create found it. */
void spcbpt_viewer_destroy(spcbpt_viewer* v);
int spcbpt_viewer_mouse_button(spcbpt_viewer* v, int button, int action, double x, double y);
int spcbpt_viewer_cursor_pos(spcbpt_viewer* v, double x, double y);
int spcbpt_viewer_scroll(spcbpt_viewer* v, double xscroll, double yscroll);
int spcbpt_viewer_window_size(spcbpt_viewer* v, int width, int height);
int spcbpt_viewer_iconify(spcbpt_viewer* v, int iconified);
int spcbpt_viewer_key(spcbpt_viewer* v, int key, int action);
int spcbpt_viewer_set_fps(spcbpt_viewer* v, float fps);
/* How far the loop runs ahead of what it shows (the reference has no such modes; every mode shows the SAME frames -- same launch
 * frames, same caches, same images, tests/test_viewer.py):
 *   0  the reference's order: light pass, sampler build, eye launch, device sync, strictly in turn (optixPathTracer.cpp:791-822);
 *   1  with "SPCBPT_eye" the NEXT frame's light pass is launched right after this frame's eye launch, before the sync, so that it
 *      runs beside the eye kernel (light sub-paths do not depend on the camera);
 *   2  (default) the next frame is traced while this one is shown: its sampler build and its eye launch WITHOUT the film merge
 *      (spcbpt_launch_deferred) are queued before spcbpt_viewer_frame returns, which waits for the shown frame's merge only
 *      (spcbpt_sync_film).  The next call merges that frame if nothing it depends on has changed since -- camera, size, algorithm,
 *      subframe restart -- and drops it otherwise; light pass and sampler are kept either way, so the k-th "SPCBPT_eye" frame
 *      always uses the k-th light pass.  Only a call that saw NO event speculates: while the camera is dragged (every call sees a
 *      change) the loop runs as mode 1 -- no frame is queued just to be dropped by the next event -- and the first steady call
 *      starts tracing ahead again.  A steady view costs the eye kernel per displayed frame.
 * Modes 1 and 2 set spcbpt_set_light_ahead on the context; spcbpt_viewer_destroy drops what the viewer queued ahead and restores the
 * mode it found, so a host can go on with the plain loop on the same context (destroy the viewer BEFORE its context: it calls into it).  A host that touches the context BETWEEN two
 * viewer frames (merges / drops the deferred frame, new tuple, sky, cache import) is tolerated: each frame re-validates the viewer's
 * flags against spcbpt_get_pipeline_state.  To DISPLAY a frame read it with spcbpt_read_film (or spcbpt_accum_device_ptr after
 * spcbpt_viewer_frame): spcbpt_read_frame / _accum wait for everything queued, i.e. also for the frame being traced ahead.
 * spcbpt_viewer_set_light_ahead(v, on) = set_pipeline(v, on ? 1 : 0). */
int spcbpt_viewer_set_pipeline(spcbpt_viewer* v, int mode);
int spcbpt_viewer_set_light_ahead(spcbpt_viewer* v, int on);
/* History reprojection in the loop (spcbpt_history_*; off by default, and then nothing of it is called).  While on:
 *   - every subframe-0 frame is followed by spcbpt_launch_features(ctx, 0, ...), the centre rays' first hits;
 *   - a frame that saw a camera change and nothing else -- no resize, no algorithm switch, no P restart -- with at least one frame
 *     shown under the old camera drops the frame traced ahead as always, calls spcbpt_history_capture(ctx, frames shown so far)
 *     before spcbpt_set_camera, and queues spcbpt_history_reproject with the defaults behind the features of the new view;
 *   - every shown frame is followed by spcbpt_history_resolve(ctx, subframe_index + 1), behind that frame's merge and, in mode 2, in
 *     front of spcbpt_launch_deferred.  What to display is then spcbpt_read_history's resolved image; the film is what it always was.
 * Any other restart (resize, algorithm switch, P) and flipping the switch call spcbpt_history_reset; flipping the switch also
 * restarts the accumulation.  The three pipeline modes show the same resolved frames.  With a null context the switch is state
 * only.  `live` tells whether a prior is live on the context, i.e. whether the resolved image differs from the film. */
int spcbpt_viewer_set_reproject(spcbpt_viewer* v, int on);
int spcbpt_viewer_get_reproject(spcbpt_viewer* v, int* on, int* live);
/* Denoising what the loop shows (spcbpt_history_denoise; off by default).  Needs the reproject switch on (else SPCBPT_ERR_STATE);
 * switching reproject off switches it off.  Switching it on switches the context's film moments on, switching it off restores what
 * it found; flipping it restarts the accumulation like spcbpt_viewer_set_reproject.  While on, every shown frame's
 * spcbpt_history_resolve is followed by spcbpt_history_denoise with the default parameters (in every pipeline mode in front of the
 * deferred launch), and what to display is spcbpt_read_denoised.  The film is what it always was. */
int spcbpt_viewer_set_denoise(spcbpt_viewer* v, int on);
int spcbpt_viewer_get_denoise(spcbpt_viewer* v, int* on);
int spcbpt_viewer_frame(spcbpt_viewer* v);
int spcbpt_viewer_get_state(spcbpt_viewer* v, spcbpt_viewer_state* state);
const char* spcbpt_viewer_alg_name(int alg_id);

/* Read back the installed subspace tuple (checkpoint writer the reference lacks). */
int spcbpt_get_subspace(spcbpt_ctx* ctx,
                        spcbpt_tree_node* eye_tree, int* n_eye, int cap_eye,
                        spcbpt_tree_node* light_tree, int* n_light, int cap_light,
                        float* q, float* cmf_gamma);

/* `.scene` + OBJ ingestion: replaces LoadScene (OptiXPathTracer/sceneLoader.cpp:47-308) and the
 * flattening Scene_shift does (OptiXPathTracer/scene_shift.cpp:32-328).  data_root plays SAMPLES_DIR "/data": mesh and
 * texture paths of the file are relative to it (back-slashes accepted).  The desc points into the handle's storage
 * and stays valid until spcbpt_scene_file_free.  Needs no GPU. */
typedef struct spcbpt_scene_file spcbpt_scene_file;
int spcbpt_scene_file_load(const char* scene_path, const char* data_root, spcbpt_scene_file** out);
/* glTF 2.0 (.gltf with external / base64 buffers, or .glb) into the same handle, read the way the reference's own glTF route
 * reads it (sutil::loadScene + processGLTFNode, sutil/Scene.cpp:119-210, 266-550; never called by the reference app): root
 * nodes = nodes without a parent, transform = parent * matrix^T * T * R * S in fp32, TRIANGLES primitives with POSITION /
 * TEXCOORD_0 / indices, baseColor / metallic / roughness factors, baseColorTexture (binary PPM images only), first perspective
 * camera.  Quad lights come from the caller or from this build's root `extras.spcbpt_quad_lights`; emissive materials are
 * handed out as mesh lights by spcbpt_scene_file_mesh_lights.  On failure the message
 * is written to `error` (may be NULL). */
int spcbpt_gltf_load(const char* path, spcbpt_scene_file** out, char* error, int error_capacity);
int spcbpt_scene_file_desc(spcbpt_scene_file* s, spcbpt_scene_desc* desc);
int spcbpt_scene_file_camera(spcbpt_scene_file* s, float eye[3], float lookat[3], float up[3], float* fov_y_deg,
                             int* width, int* height);
/* The scene's environment map: `env_file` of the cameraSetting block (sceneLoader.cpp:242), read like HDRLoader does (width = 0: the
 * scene names none, or it could not be read: see the warnings), and the sky.center / sky.r env_params_setup would derive from
 * the reference's scene box (optixPathTracer.cpp:458-459; SURVEY q7: only the first third of every OBJ shape's vertices enters it)
 * -- to be handed to spcbpt_set_environment.  The pointers stay valid until spcbpt_scene_file_free. */
int spcbpt_scene_file_environment(spcbpt_scene_file* scene, const float** rgba, int* width, int* height, float center[3], float* radius);
/* The mesh lights of a glTF file: one per material with a non-zero `emissiveFactor` that some triangle uses, emission =
 * emissiveFactor x KHR_materials_emissive_strength.emissiveStrength (default 1) -- what sutil/Scene.cpp:1739-1743 tests, completed
 * by spcbpt_create_lit.  n_patches = root `extras.spcbpt_mesh_light_patches` (default 4), reduced so that quads and mesh lights fit
 * the 200 patch subspaces.  emissiveTexture and doubleSided are not honoured (a line in the warnings).  What spcbpt_scene_file_desc
 * returns does not depend on them; a `.scene` file has none.  The pointer stays valid until spcbpt_scene_file_free. */
int spcbpt_scene_file_mesh_lights(spcbpt_scene_file* s, const spcbpt_mesh_light** mesh_lights, int* n_mesh_lights);
const char* spcbpt_scene_file_warnings(spcbpt_scene_file* s);
int spcbpt_scene_file_free(spcbpt_scene_file* s);

/* Scene statistics after create. */
int spcbpt_scene_info(spcbpt_ctx* ctx, int* n_triangles, int* n_bvh_nodes, int* bvh_depth);

#ifdef __cplusplus
}
#endif
#endif /* SPCBPT_H */
