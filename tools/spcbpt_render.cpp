// Headless driver over the C ABI: the frame sequence of the reference app (OptiXPathTracer/optixPathTracer.cpp main 680-837,
// preprocessing 552-608, render loop 791-822) without GLFW/GL — loads a `.scene`, builds the LBVH, runs the preprocessing,
// renders N subframes of "pt", "SPCBPT_eye" or "lt" and writes the linear accum buffer as PFM and the tone-mapped frame as PPM.  A scene
// that names an `env_file` gets its sky (spcbpt_set_environment); --env-mode N sets spcbpt_set_environment_mode (SPCBPT_ENV_* bits).
// --emissive: the emissive materials of a glTF file light the scene as mesh lights (spcbpt_create_lit); with them a file needs no quad.
// --alg lt: light tracing (the light-vertex cache splatted onto the film): a light pass and a sampler build per frame over the minimal
// tuple, no preprocessing; its Mpaths/s line counts the light paths only.  --ordered-splat: "lt" sums every pixel's contributions in cache
// order (spcbpt_set_splat_order(ctx, SPCBPT_SPLAT_ORDERED)): two runs write the same bytes.
// --denoise: a first-hit feature launch beside every frame and one a-trous denoise (spcbpt_denoise, default parameters) after the last;
// writes <out>_denoised.pfm / .ppm next to the usual files.  --features: writes the feature buffers as <out>_albedo.pfm,
// <out>_normal.pfm and <out>_depth.pfm (depth in all three channels).
// --guides [N]: with --denoise / --denoise-variance a reflected-guide launch (spcbpt_launch_guides; up to N mirrors, default
// SPCBPT_GUIDE_MAX_BOUNCES, the other parameters at their defaults) beside the features of every frame, and the denoiser reads those planes
// (spcbpt_set_denoise_guides); with --features also <out>_guide_albedo.pfm, <out>_guide_normal_depth.pfm (the unfolded normal) and
// <out>_guide_depth.pfm (the unfolded path length in all three channels).  Without the flag every output file keeps its bytes.
// --denoise-variance: the same with the variance-guided filter (spcbpt_denoise_variance; switches the film's moments on).
// --target-error E [--check-every K]: switches the film's moments on and renders until spcbpt_film_error's mean is <= E (asked every K
// frames, default 8, from the second frame on) or --frames is reached; prints the frames used and the error reached.
// --aperture R [--focus F]: a thin-lens camera (spcbpt_set_lens) of radius R in world units, focused at depth F in units of the distance to
// the camera's lookat point (default 1); "pt", "SPCBPT_eye" and "lt" render through it, --adaptive is refused by the library.
// --adaptive (with --alg SPCBPT_eye and --target-error E) [--min-samples M] [--max-samples X] [--check-every K]: adaptive sampling.
// max(M, 2) uniform frames, spcbpt_adaptive_begin, then rounds of spcbpt_adaptive_select followed by up to K (default 1) times (light
// pass, sampler build, spcbpt_launch_adaptive) until the selection is empty or a tile would pass min(X, --frames) samples; prints the
// tile-samples traced next to tiles x frames and writes the per-tile sample counts as <out>_samples.pgm (one pixel per 8x8 tile).
// --robust K [--robust-strength S]: the bucket film (spcbpt_set_film_buckets(ctx, K), K = 3 .. 32) beside the film and one
// spcbpt_robust_resolve (strength S in [0, 8], default 1) after the last frame; writes <out>_robust.pfm / .ppm next to the usual files.
// Not with --adaptive (the per-tile merge fills no buckets).
// --exposure EV | --auto-exposure [--key K], --tone film|reinhard|aces|linear: the display transform (spcbpt_display) of the last image
// the run produced -- the robust image, else the denoised one, else the film -- at a manual EV (default 0) or at the EV measured from
// that image's luminance histogram (key K, default 0.18), through the tone operator (default film); writes <out>_display.ppm next to
// the usual files, which stay as they are, and prints the EV used.
// --bloom S [--bloom-levels N] [--bloom-threshold T]: that image goes through spcbpt_bloom first (strength S in [0, 1], N = 1 .. 8 levels,
// default 5, luminance threshold T, default 0) and the bloom plane is what <out>_display.ppm shows; --bloom alone implies the display
// pass with its defaults.  <out>.pfm and <out>.ppm keep their bytes.
// --local-tone C [--local-detail D] [--local-cell S] [--local-range R]: that image -- after --bloom, if given -- goes through
// spcbpt_local_tone (compress C in (0, 2], detail D, default 1, S = 4 .. 64 pixels per grid cell, default 16, R stops per bin, default 1)
// and the local tone plane is what <out>_display.ppm shows; --local-tone alone implies the display pass with its defaults.
// --batch N (with --alg SPCBPT_eye; N = 2 .. 32): the uniform frames in groups of up to N -- the group's light passes as one launch
// (spcbpt_launch_light_batch, the launch frames the per-frame loop uses), their sampler builds as one (spcbpt_build_sampler_batch) and one
// spcbpt_launch_eye_batch_film, whose merge keeps the moments and the buckets -- so --target-error (asked after a group; --check-every
// is rounded up to a multiple of N), --denoise-variance, --robust and the uniform phase of --adaptive run at the batched loop's rate.
// The files are bit for bit those of the same command without --batch that renders as many frames.  Not with --features, --denoise,
// --aperture or another algorithm: their per-frame launches have no batched form.
//   spcbpt_render <file.scene> <data_root> [--alg pt|SPCBPT_eye|lt] [--dim=WxH] [--frames N] [--train-paths N] [--minimal] [--env-mode N] [--emissive] [--aperture R] [--focus F] [--ordered-splat] [--denoise] [--denoise-variance] [--features] [--target-error E] [--check-every K] [--adaptive] [--min-samples M] [--max-samples X] [--robust K] [--robust-strength S] [--exposure EV] [--auto-exposure] [--tone film|reinhard|aces|linear] [--key K] [--bloom S] [--bloom-levels N] [--bloom-threshold T] [--local-tone C] [--local-detail D] [--local-cell S] [--local-range R] [--batch N] [--out prefix]
// Build: make -C tools   (links libspcbpt_hip.so)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/spcbpt.h"

static void die(spcbpt_ctx* c, const char* what, int rc) {
    fprintf(stderr, "%s failed (%d): %s\n", what, rc, spcbpt_last_error(c));
    exit(1);  // optixPathTracer.cpp:830-834: print and return 1
}
#define CHECK(c, call) do { int rc__ = (call); if (rc__) die(c, #call, rc__); } while (0)

// PFM: bottom row first, which is exactly the accum_buffer orientation; channels c0, c1, c2 of a float4 image
static void write_pfm(const std::string& path, const std::vector<float>& rgba, int width, int height, int c0 = 0, int c1 = 1, int c2 = 2) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(1); }
    fprintf(f, "PF\n%d %d\n-1.0\n", width, height);
    for (size_t i = 0; i < (size_t)width * height; i++) {
        const float px[3] = {rgba[4 * i + c0], rgba[4 * i + c1], rgba[4 * i + c2]};
        fwrite(px, 4, 3, f);
    }
    fclose(f);
}
// PPM: top row first
static void write_ppm(const std::string& path, const std::vector<uint8_t>& rgba8, int width, int height) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(1); }
    fprintf(f, "P6\n%d %d\n255\n", width, height);
    for (int y = height - 1; y >= 0; y--)
        for (int x = 0; x < width; x++) fwrite(&rgba8[4 * ((size_t)y * width + x)], 1, 3, f);
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s <file.scene | file.gltf | file.glb> <data_root (ignored for glTF)> [--alg pt|SPCBPT_eye|lt] [--dim=WxH] [--frames N] [--train-paths N] [--minimal] [--env-mode N] [--emissive] [--aperture R] [--focus F] [--ordered-splat] [--denoise] [--denoise-variance] [--features] [--guides [N]] [--target-error E] [--check-every K] [--adaptive] [--min-samples M] [--max-samples X] [--robust K] [--robust-strength S] [--exposure EV] [--auto-exposure] [--tone film|reinhard|aces|linear] [--key K] [--bloom S] [--bloom-levels N] [--bloom-threshold T] [--local-tone C] [--local-detail D] [--local-cell S] [--local-range R] [--batch N] [--out prefix]\n", argv[0]);
        return 0;
    }
    std::string alg = "SPCBPT_eye", out = "render";
    int width = 1920, height = 1000, frames = 16, train_paths = 2000000;  // optixPathTracer.cpp:84-85 default size
    int env_mode = 0;
    bool minimal = false, emissive = false, ordered_splat = false, denoise = false, features = false, denoise_variance = false, guides = false;
    spcbpt_guide_params gp = {SPCBPT_GUIDE_MAX_BOUNCES, SPCBPT_GUIDE_ROUGHNESS_MAX, SPCBPT_GUIDE_METALLIC_MIN};
    double target_error = 0.0;   // > 0: stop once the film's mean relative standard error is there
    int check_every = 8;
    bool adaptive = false, check_every_given = false;
    int min_samples = 0, max_samples = 0;
    int robust = 0;               // > 0: the number of buckets
    float robust_strength = 1.0f;
    bool display = false;         // any of --exposure / --auto-exposure / --tone / --key
    spcbpt_display_params disp;
    spcbpt_display_default_params(&disp);
    bool bloom = false;           // --bloom S: the shown image goes through spcbpt_bloom first
    spcbpt_bloom_params blm;
    spcbpt_bloom_default_params(&blm);
    bool local_tone = false;      // --local-tone C: the shown image goes through spcbpt_local_tone (after spcbpt_bloom, if both)
    spcbpt_local_tone_params ltp;
    spcbpt_local_tone_default_params(&ltp);
    int batch = 0;                // --batch N: the uniform frames in groups of up to N (one batched eye launch per group)
    float aperture = 0.0f, focus = 1.0f;   // --aperture R [--focus F]: a thin lens of radius R (world units) focused at depth F (1 = the lookat plane)
    for (int i = 3; i < argc; i++) {
        std::string a = argv[i];
        if (a == "--alg" && i + 1 < argc) alg = argv[++i];
        else if (a.rfind("--dim=", 0) == 0) { if (sscanf(a.c_str() + 6, "%dx%d", &width, &height) != 2) { fprintf(stderr, "bad --dim\n"); return 1; } }
        else if (a == "--frames" && i + 1 < argc) frames = atoi(argv[++i]);
        else if (a == "--train-paths" && i + 1 < argc) train_paths = atoi(argv[++i]);
        else if (a == "--minimal") minimal = true;
        else if (a == "--env-mode" && i + 1 < argc) env_mode = atoi(argv[++i]);
        else if (a == "--emissive") emissive = true;
        else if (a == "--ordered-splat") ordered_splat = true;
        else if (a == "--denoise") denoise = true;
        else if (a == "--denoise-variance") denoise = denoise_variance = true;
        else if (a == "--features") features = true;
        else if (a == "--guides") { guides = true; if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') gp.max_bounces = atoi(argv[++i]); }
        else if (a == "--target-error" && i + 1 < argc) target_error = atof(argv[++i]);
        else if (a == "--check-every" && i + 1 < argc) { check_every = atoi(argv[++i]); check_every_given = true; }
        else if (a == "--adaptive") adaptive = true;
        else if (a == "--min-samples" && i + 1 < argc) min_samples = atoi(argv[++i]);
        else if (a == "--max-samples" && i + 1 < argc) max_samples = atoi(argv[++i]);
        else if (a == "--robust" && i + 1 < argc) robust = atoi(argv[++i]);
        else if (a == "--robust-strength" && i + 1 < argc) robust_strength = (float)atof(argv[++i]);
        else if (a == "--exposure" && i + 1 < argc) { disp.ev = (float)atof(argv[++i]); display = true; }
        else if (a == "--auto-exposure") { disp.flags |= SPCBPT_DISPLAY_AUTO; display = true; }
        else if (a == "--key" && i + 1 < argc) { disp.key = (float)atof(argv[++i]); display = true; }
        else if (a == "--tone" && i + 1 < argc) {
            const std::string t = argv[++i];
            if (t == "film") disp.op = SPCBPT_TONE_FILM;
            else if (t == "reinhard") disp.op = SPCBPT_TONE_REINHARD;
            else if (t == "aces") disp.op = SPCBPT_TONE_ACES;
            else if (t == "linear") disp.op = SPCBPT_TONE_LINEAR;
            else { fprintf(stderr, "--tone takes film, reinhard, aces or linear\n"); return 1; }
            display = true;
        }
        else if (a == "--bloom" && i + 1 < argc) { blm.strength = (float)atof(argv[++i]); bloom = true; display = true; }
        else if (a == "--bloom-levels" && i + 1 < argc) blm.levels = atoi(argv[++i]);
        else if (a == "--bloom-threshold" && i + 1 < argc) blm.threshold = (float)atof(argv[++i]);
        else if (a == "--local-tone" && i + 1 < argc) { ltp.compress = (float)atof(argv[++i]); local_tone = true; display = true; }
        else if (a == "--local-detail" && i + 1 < argc) ltp.detail = (float)atof(argv[++i]);
        else if (a == "--local-cell" && i + 1 < argc) ltp.cell = atoi(argv[++i]);
        else if (a == "--local-range" && i + 1 < argc) ltp.range = (float)atof(argv[++i]);
        else if (a == "--aperture" && i + 1 < argc) aperture = (float)atof(argv[++i]);
        else if (a == "--focus" && i + 1 < argc) focus = (float)atof(argv[++i]);
        else if (a == "--batch" && i + 1 < argc) { batch = atoi(argv[++i]); if (batch == 0) batch = -1; }
        else if (a == "--out" && i + 1 < argc) out = argv[++i];
        else { fprintf(stderr, "Unknown option '%s'\n", argv[i]); return 1; }
    }
    if (adaptive && (alg != "SPCBPT_eye" || !(target_error > 0.0) || min_samples < 0 || max_samples < 0)) {
        fprintf(stderr, "--adaptive needs --alg SPCBPT_eye and --target-error E > 0 (and non-negative --min-samples / --max-samples)\n");
        return 1;
    }
    if (adaptive && !check_every_given) check_every = 1;
    if (robust != 0 && (adaptive || robust < 3 || robust > 32)) {
        fprintf(stderr, "--robust K needs K in 3 .. 32 and no --adaptive\n");
        return 1;
    }
    if (batch != 0) {
        if (batch < 2 || batch > 32) { fprintf(stderr, "--batch N needs N in 2 .. 32\n"); return 1; }
        const char* why = alg != "SPCBPT_eye" ? "--alg other than SPCBPT_eye" : features ? "--features" : (denoise && !denoise_variance) ? "--denoise" : aperture != 0.0f ? "--aperture" : nullptr;
        if (why) {
            fprintf(stderr, "--batch: not with %s: its per-frame launches have no batched form (the batched eye kernel renders pinhole \"SPCBPT_eye\" frames, "
                            "and the feature buffers of --features / --denoise are kept per frame)\n", why);
            return 1;
        }
        char n[16];
        snprintf(n, sizeof(n), "%d", batch);
        setenv("SPCBPT_EYE_BATCH", n, 1);   // read by spcbpt_create: sizes the ring of sampler buffer sets for batches of N
    }
    spcbpt_scene_file* sf = nullptr;
    const std::string in(argv[1]);
    const bool gltf = in.size() > 5 && (in.compare(in.size() - 5, 5, ".gltf") == 0 || in.compare(in.size() - 4, 4, ".glb") == 0);
    char load_err[512] = {0};
    if (gltf ? spcbpt_gltf_load(argv[1], &sf, load_err, sizeof(load_err)) : spcbpt_scene_file_load(argv[1], argv[2], &sf)) {
        fprintf(stderr, "cannot read %s %s\n", argv[1], load_err);
        return 1;
    }
    if (*spcbpt_scene_file_warnings(sf)) fprintf(stderr, "scene warnings: %s\n", spcbpt_scene_file_warnings(sf));
    spcbpt_scene_desc desc;
    spcbpt_scene_file_desc(sf, &desc);
    float eye[3], lookat[3], up[3], fov;
    spcbpt_scene_file_camera(sf, eye, lookat, up, &fov, nullptr, nullptr);
    spcbpt_ctx* ctx = nullptr;
    const spcbpt_mesh_light* mesh_lights = nullptr;
    int n_mesh_lights = 0;
    if (emissive) spcbpt_scene_file_mesh_lights(sf, &mesh_lights, &n_mesh_lights);
    if (emissive && n_mesh_lights == 0) fprintf(stderr, "--emissive: the file has no emissive material in use\n");
    int rc = n_mesh_lights > 0 ? spcbpt_create_lit(&desc, mesh_lights, n_mesh_lights, 0, &ctx) : spcbpt_create(&desc, 0, &ctx);
    if (rc) die(nullptr, "spcbpt_create", rc);
    for (int k = 0; k < n_mesh_lights; k++) {
        int32_t type = 0, tris = 0, first = 0, patches = 0;
        float area = 0.0f;
        CHECK(ctx, spcbpt_light_info(ctx, desc.n_lights + k, &type, &area, &tris, &first, &patches));
        printf("mesh light %d: material %d, %d triangles, area %g, %d patch subspaces from %d down\n", k, mesh_lights[k].material, tris, area, patches, first);
    }
    int nt, nn, depth;
    CHECK(ctx, spcbpt_scene_info(ctx, &nt, &nn, &depth));
    printf("scene: %d triangles, BVH %d nodes depth %d\n", nt, nn, depth);
    {   // the scene's env_file, if it names one (env_params_setup, optixPathTracer.cpp:431-461)
        const float* rgba = nullptr;
        int ew = 0, eh = 0;
        float center[3], radius = 0.0f;
        if (spcbpt_scene_file_environment(sf, &rgba, &ew, &eh, center, &radius) == SPCBPT_OK && rgba && ew > 0) {
            CHECK(ctx, spcbpt_set_environment(ctx, rgba, ew, eh, center, radius));
            printf("environment map: %dx%d\n", ew, eh);
        }
    }
    CHECK(ctx, spcbpt_set_environment_mode(ctx, env_mode));
    CHECK(ctx, spcbpt_set_camera_lookat(ctx, eye, lookat, up, fov, (float)width / (float)height));
    CHECK(ctx, spcbpt_resize(ctx, width, height));
    if (aperture != 0.0f) {   // (a bad value is the library's to refuse; so is --adaptive, which has no lens form)
        CHECK(ctx, spcbpt_set_lens(ctx, aperture, focus));
        printf("lens: radius %g, focus %g\n", aperture, focus);
    }
    if (ordered_splat) {
        CHECK(ctx, spcbpt_set_splat_order(ctx, SPCBPT_SPLAT_ORDERED));
        printf("splat order: ordered (the film of \"lt\" is bit-reproducible)\n");
    }
    const bool moments = denoise_variance || target_error > 0.0;
    if (moments) CHECK(ctx, spcbpt_set_film_moments(ctx, 1));
    if (robust) CHECK(ctx, spcbpt_set_film_buckets(ctx, robust));
    if (check_every < 1) check_every = 1;
    if (batch) check_every = (check_every + batch - 1) / batch * batch;   // the film error is asked after a group
    spcbpt_light_trace_params lt = {100000, 52, 1, 0, 0, 1};
    CHECK(ctx, spcbpt_set_light_trace(ctx, &lt));
    auto t0 = std::chrono::steady_clock::now();
    const bool lt_alg = alg == "lt";
    if (lt_alg) CHECK(ctx, spcbpt_set_subspace(ctx, nullptr, 0, nullptr, 0, nullptr, nullptr));   // the light pass labels its vertices; "lt" reads no label
    if (alg == "SPCBPT_eye") {
        if (minimal) CHECK(ctx, spcbpt_set_subspace(ctx, nullptr, 0, nullptr, 0, nullptr, nullptr));
        else CHECK(ctx, spcbpt_preprocess(ctx, train_paths, train_paths, 1));
    }
    auto t1 = std::chrono::steady_clock::now();
    printf("preprocessing: %.2f s\n", std::chrono::duration<double>(t1 - t0).count());
    spcbpt_film_error_stats reached = {0, 0.0, 0.0};
    unsigned lt_frame = 1000000;  // continues after the Q passes of the preprocessing like lt_params.launch_frame
    // --adaptive: the uniform frames the estimate needs, then only the tiles that are still above the target
    const int cap = adaptive ? (max_samples > 0 && max_samples < frames ? max_samples : frames) : 0;   // samples no tile passes
    const int uniform_frames = adaptive ? std::min(cap, std::max(min_samples, 2)) : frames;
    if (batch) {   // the uniform frames in groups: light passes, sampler builds and the eye launch of a group as one launch each
        // The loop of bench.py: the light passes run two groups ahead of the eye launch and the builds one -- a batched light pass is a
        // thin grid meant to run BESIDE an eye kernel, and a group's builds run under the eye kernel of the group before.  Frame f keeps
        // launch frame lt_frame + 1 + f, the one the loop below gives it.  (A run that stops at its target leaves the work ahead unused.)
        CHECK(ctx, spcbpt_set_light_ahead(ctx, 1));   // (the batched light pass queues its passes for the builds)
        const unsigned light0 = lt_frame + 1;
        int lit = 0, built = 0;   // frames whose light pass has been launched / whose sampler has been built
        auto light_next = [&]() {
            const int g = std::min(batch, uniform_frames - lit);
            if (g <= 0) return;
            // (the first group has no eye kernel to run beside and everything waits for it: full-size single passes, which leave the
            // same caches in the same queue, are done sooner than the thin grid of a batched pass)
            if (lit == 0) for (int k = 0; k < g; k++) CHECK(ctx, spcbpt_launch(ctx, "light trace", light0 + (unsigned)k, 0, 0, 1));
            else CHECK(ctx, spcbpt_launch_light_batch(ctx, light0 + (unsigned)lit, g));
            lit += g;
        };
        auto build_next = [&]() {
            const int g = std::min(batch, lit - built);
            if (g > 0) { CHECK(ctx, spcbpt_build_sampler_batch(ctx, g)); built += g; }
        };
        light_next(); build_next(); light_next();
        for (int f = 0; f < uniform_frames;) {
            const int g = std::min(batch, uniform_frames - f);
            uint32_t subframes[32];
            for (int k = 0; k < g; k++) subframes[k] = (uint32_t)(f + k);
            CHECK(ctx, spcbpt_launch_eye_batch_film(ctx, g, subframes, 0, height, 1));   // the samplers of the last g builds
            build_next(); light_next();
            if (denoise) for (int k = 0; k < g; k++) CHECK(ctx, spcbpt_launch_features(ctx, subframes[k], 0, height, 1));   // (--denoise-variance)
            if (denoise && guides) for (int k = 0; k < g; k++) CHECK(ctx, spcbpt_launch_guides(ctx, subframes[k], 0, height, 1, &gp));
            f += g;
            if (!adaptive && target_error > 0.0 && f >= 2 && (f % check_every == 0 || f == frames)) {
                CHECK(ctx, spcbpt_film_error(ctx, &reached));
                if (reached.pixels > 0 && reached.mean <= target_error) { frames = f; break; }
            }
        }
        CHECK(ctx, spcbpt_set_light_ahead(ctx, 0));   // (what follows -- the adaptive rounds -- builds from the latest pass again)
        lt_frame += (unsigned)uniform_frames;
    }
    else for (int f = 0; f < uniform_frames; f++) {
        if (alg == "SPCBPT_eye" || lt_alg) {  // launchLVCTrace (optixPathTracer.cpp:515-522)
            CHECK(ctx, spcbpt_launch(ctx, "light trace", ++lt_frame, 0, 0, 1));
            CHECK(ctx, spcbpt_build_sampler(ctx));
        }
        CHECK(ctx, spcbpt_launch(ctx, alg.c_str(), (uint32_t)f, 0, height, 1));  // launchSubframe (609-635)
        if (denoise || features) CHECK(ctx, spcbpt_launch_features(ctx, (uint32_t)f, 0, height, 1));   // the same subframe's primary rays
        if (guides && (denoise || features)) CHECK(ctx, spcbpt_launch_guides(ctx, (uint32_t)f, 0, height, 1, &gp));   // ... followed through the mirrors
        if (!adaptive && target_error > 0.0 && f >= 1 && ((f + 1) % check_every == 0 || f + 1 == frames)) {
            CHECK(ctx, spcbpt_film_error(ctx, &reached));
            if (reached.pixels > 0 && reached.mean <= target_error) { frames = f + 1; break; }
        }
    }
    long long tile_samples_traced = 0;
    int tiles_x = 0, tiles_y = 0;
    if (adaptive) {
        CHECK(ctx, spcbpt_adaptive_begin(ctx, (uint32_t)uniform_frames));
        CHECK(ctx, spcbpt_get_adaptive_state(ctx, nullptr, &tiles_x, &tiles_y, nullptr));
        const spcbpt_adaptive_params ap = {(float)target_error, (uint32_t)min_samples, (uint32_t)cap};
        int level = uniform_frames, rounds = 0, launches = 0, listed = 0;   // level: no tile has more samples than this
        while (level < cap) {
            CHECK(ctx, spcbpt_adaptive_select(ctx, &ap, &listed));
            if (listed == 0) break;
            rounds++;
            for (int k = 0; k < check_every && level < cap; k++, level++, launches++) {
                CHECK(ctx, spcbpt_launch(ctx, "light trace", ++lt_frame, 0, 0, 1));
                CHECK(ctx, spcbpt_build_sampler(ctx));
                CHECK(ctx, spcbpt_launch_adaptive(ctx, "SPCBPT_eye"));
                tile_samples_traced += listed;
            }
        }
        CHECK(ctx, spcbpt_film_error(ctx, &reached));
        const long long tiles = (long long)tiles_x * tiles_y, uniform = tiles * uniform_frames, full = tiles * frames;
        printf("adaptive: target error %g, %d uniform frames, %d rounds, %d adaptive launches; tile-samples traced %lld of %lld (tiles x frames = %lld x %d), %.1f %%; "
               "film error reached %.6g (max %.6g)\n", target_error, uniform_frames, rounds, launches, uniform + tile_samples_traced, full, tiles, frames,
               100.0 * (double)(uniform + tile_samples_traced) / (double)full, reached.mean, reached.max);
    }
    else if (target_error > 0.0) {
        if (frames < 2) CHECK(ctx, spcbpt_film_error(ctx, &reached));
        printf("target error %g: %d frames used, error reached %.6g (max %.6g over %lld pixels)\n", target_error, frames, reached.mean, reached.max,
               (long long)reached.pixels);
    }
    if (denoise) {
        if (guides) CHECK(ctx, spcbpt_set_denoise_guides(ctx, SPCBPT_GUIDES_REFLECTED));
        const spcbpt_denoise_params dp = {5, 0.0f, 0.0f, 0.0f};   // the defaults of include/spcbpt.h
        if (denoise_variance) CHECK(ctx, spcbpt_denoise_variance(ctx, &dp));
        else CHECK(ctx, spcbpt_denoise(ctx, &dp));
    }
    if (robust) CHECK(ctx, spcbpt_robust_resolve(ctx, robust_strength));
    const int display_source = robust ? SPCBPT_DISPLAY_ROBUST : (denoise ? SPCBPT_DISPLAY_DENOISED : SPCBPT_DISPLAY_FILM);
    if (bloom) CHECK(ctx, spcbpt_bloom(ctx, display_source, &blm));
    if (local_tone) CHECK(ctx, spcbpt_local_tone(ctx, bloom ? SPCBPT_DISPLAY_BLOOM : display_source, &ltp));
    if (display) CHECK(ctx, spcbpt_display(ctx, local_tone ? SPCBPT_DISPLAY_LOCAL : (bloom ? SPCBPT_DISPLAY_BLOOM : display_source), &disp));
    CHECK(ctx, spcbpt_sync(ctx));
    auto t2 = std::chrono::steady_clock::now();
    const double sec = std::chrono::duration<double>(t2 - t1).count();
    if (adaptive) printf("up to %d samples per tile of %s at %dx%d: %.3f s\n", cap, alg.c_str(), width, height, sec);
    else printf("%d subframes of %s at %dx%d: %.3f s, %.2f Mpaths/s\n", frames, alg.c_str(), width, height, sec,
           (lt_alg ? (double)lt.num_core : (double)width * height + (alg == "SPCBPT_eye" ? lt.num_core : 0)) * frames / sec / 1e6);
    std::vector<float> accum((size_t)width * height * 4);
    std::vector<uint8_t> frame((size_t)width * height * 4);
    CHECK(ctx, spcbpt_read_accum(ctx, accum.data()));
    CHECK(ctx, spcbpt_read_frame(ctx, frame.data()));
    write_pfm(out + ".pfm", accum, width, height);
    write_ppm(out + ".ppm", frame, width, height);
    printf("wrote %s.pfm and %s.ppm\n", out.c_str(), out.c_str());
    if (adaptive) {   // the sample-count plane: one pixel per 8x8 tile, top row first like the PPM
        std::vector<uint32_t> counts((size_t)tiles_x * tiles_y);
        CHECK(ctx, spcbpt_read_adaptive(ctx, counts.data(), nullptr, nullptr, 0, nullptr));
        uint32_t top = 1;
        for (uint32_t v : counts) top = std::max(top, v);
        if (top > 65535u) top = 65535u;
        const std::string path = out + "_samples.pgm";
        FILE* f = fopen(path.c_str(), "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", path.c_str()); return 1; }
        fprintf(f, "P5\n%d %d\n%u\n", tiles_x, tiles_y, top);
        for (int y = tiles_y - 1; y >= 0; y--)
            for (int x = 0; x < tiles_x; x++) {
                const uint32_t v = std::min(counts[(size_t)y * tiles_x + x], top);
                const uint8_t b[2] = {(uint8_t)(v >> 8), (uint8_t)(v & 255u)};
                if (top > 255u) fwrite(b, 1, 2, f); else fwrite(b + 1, 1, 1, f);
            }
        fclose(f);
        printf("wrote %s (samples per 8x8 tile, %d x %d tiles, at most %u)\n", path.c_str(), tiles_x, tiles_y, top);
    }
    if (denoise) {
        CHECK(ctx, spcbpt_read_denoised(ctx, accum.data(), frame.data()));
        write_pfm(out + "_denoised.pfm", accum, width, height);
        write_ppm(out + "_denoised.ppm", frame, width, height);
        printf("wrote %s_denoised.pfm and %s_denoised.ppm\n", out.c_str(), out.c_str());
    }
    if (robust) {
        CHECK(ctx, spcbpt_read_robust(ctx, accum.data(), reinterpret_cast<uint32_t*>(frame.data())));
        write_pfm(out + "_robust.pfm", accum, width, height);
        write_ppm(out + "_robust.ppm", frame, width, height);
        printf("wrote %s_robust.pfm and %s_robust.ppm (%d buckets, strength %g)\n", out.c_str(), out.c_str(), robust, robust_strength);
    }
    if (display) {
        float ev = 0.0f;
        CHECK(ctx, spcbpt_read_display(ctx, frame.data(), nullptr, &ev, nullptr, nullptr));
        write_ppm(out + "_display.ppm", frame, width, height);
        static const char* const tones[] = {"film", "reinhard", "aces", "linear"};
        printf("wrote %s_display.ppm (%s, tone %s, %s EV %.9g)\n", out.c_str(), robust ? "the robust image" : (denoise ? "the denoised image" : "the film"), tones[disp.op],
               (disp.flags & SPCBPT_DISPLAY_AUTO) ? "auto" : "manual", ev);
        if (bloom) printf("  through spcbpt_bloom: strength %g, %d levels, threshold %g\n", blm.strength, blm.levels, blm.threshold);
        if (local_tone) printf("  through spcbpt_local_tone: compress %g, detail %g, cell %d, range %g\n", ltp.compress, ltp.detail, ltp.cell, ltp.range);
    }
    if (features) {
        std::vector<float> normal_depth((size_t)width * height * 4);
        CHECK(ctx, spcbpt_read_features(ctx, accum.data(), normal_depth.data()));
        write_pfm(out + "_albedo.pfm", accum, width, height);
        write_pfm(out + "_normal.pfm", normal_depth, width, height);
        write_pfm(out + "_depth.pfm", normal_depth, width, height, 3, 3, 3);
        printf("wrote %s_albedo.pfm, %s_normal.pfm and %s_depth.pfm\n", out.c_str(), out.c_str(), out.c_str());
        if (guides) {
            CHECK(ctx, spcbpt_read_guides(ctx, accum.data(), normal_depth.data()));
            write_pfm(out + "_guide_albedo.pfm", accum, width, height);
            write_pfm(out + "_guide_normal_depth.pfm", normal_depth, width, height);
            write_pfm(out + "_guide_depth.pfm", normal_depth, width, height, 3, 3, 3);
            printf("wrote %s_guide_albedo.pfm, %s_guide_normal_depth.pfm and %s_guide_depth.pfm (up to %d mirrors)\n", out.c_str(), out.c_str(), out.c_str(), gp.max_bounces);
        }
    }
    spcbpt_destroy(ctx);
    spcbpt_scene_file_free(sf);
    return 0;
}
