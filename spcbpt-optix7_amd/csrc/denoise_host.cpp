// spcbpt_denoise_host / spcbpt_denoise_variance_host / spcbpt_history_denoise_host: the denoisers of spcbpt_denoise /
// spcbpt_denoise_variance / spcbpt_history_denoise on caller buffers, on
// the host -- denoise_pixel.h, the header the kernels of kernels_denoise.hip run, over plain arrays.  No context, no GPU (plain g++,
// -ffp-contract=off like the device code).
#include <cstring>
#include <vector>

#include "../../include/spcbpt.h"
#include "denoise_pixel.h"

namespace {

struct HostPlanes {   // atrous_pixel's F over the three guide planes, 3 floats per pixel each
    const float *c, *n, *X;
    int width;
    void fetch(int x, int y, float* cq, float* nq, float* Xq) const {
        const size_t i = ((size_t)y * width + x) * 3;
        for (int k = 0; k < 3; k++) { cq[k] = c[i + k]; nq[k] = n[i + k]; Xq[k] = X[i + k]; }
    }
};

struct HostVarPlanes : HostPlanes {   // atrous_var_pixel's F: the variance plane beside them, 1 float per pixel
    const float* v;
    float variance(int x, int y) const { return v[(size_t)y * width + x]; }
};

// the demodulated film, the normals and the positions of the covered pixels; returns the diagonal of the positions' bounding box
float host_guides(const float* accum_rgba, const float* albedo_rgba, const float* normal_depth_rgba, const float* U, const float* V, const float* W,
                  int width, int height, std::vector<float>& c, std::vector<float>& n, std::vector<float>& X) {
    using namespace spc;
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    bool any = false;
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const size_t i = (size_t)y * width + x;
            denoise_demodulate(accum_rgba + i * 4, albedo_rgba + i * 4, &c[i * 3]);
            for (int k = 0; k < 3; k++) n[i * 3 + k] = normal_depth_rgba[i * 4 + k];
            denoise_position(U, V, W, width, height, x, y, normal_depth_rgba[i * 4 + 3], &X[i * 3]);
            if (albedo_rgba[i * 4 + 3] > 0.0f) {
                for (int k = 0; k < 3; k++) {
                    const float v = X[i * 3 + k];
                    lo[k] = any ? (v < lo[k] ? v : lo[k]) : v;
                    hi[k] = any ? (v > hi[k] ? v : hi[k]) : v;
                }
                any = true;
            }
        }
    return sqrtf((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
}

// the iterations and the remodulation both variance-guided forms share: c, v are the start values
int host_variance_filter(std::vector<float>& c, std::vector<float>& v, const std::vector<float>& n, const std::vector<float>& X, float diag,
                         const float* albedo_rgba, int width, int height, const spcbpt_denoise_params* p, float* out_rgba) {
    using namespace spc;
    const size_t px = (size_t)width * height;
    std::vector<float> c2(px * 3), v2(px);
    const float sigma_v = p->sigma_c > 0.0f ? p->sigma_c : SPCBPT_DENOISE_SIGMA_V;
    const float sigma_n = p->sigma_n > 0.0f ? p->sigma_n : SPCBPT_DENOISE_SIGMA_N;
    const float sigma_x = p->sigma_x > 0.0f ? p->sigma_x : SPCBPT_DENOISE_SIGMA_X_FRACTION * (diag > 0.0f ? diag : 1.0f);
    for (int it = 0; it < p->iterations; it++) {
        const AtrousVarStep a = atrous_var_step(it, sigma_v, sigma_n, sigma_x);
        HostVarPlanes f;
        f.c = c.data(); f.n = n.data(); f.X = X.data(); f.width = width; f.v = v.data();
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) {
                const size_t i = (size_t)y * width + x;
                float o[4];
                atrous_var_pixel(f, x, y, width, height, a, o);
                for (int k = 0; k < 3; k++) c2[i * 3 + k] = o[k];
                v2[i] = o[3];
            }
        c.swap(c2);
        v.swap(v2);
    }
    for (size_t i = 0; i < px; i++) {
        denoise_remodulate(&c[i * 3], albedo_rgba + i * 4, out_rgba + i * 4);
        out_rgba[i * 4 + 3] = 1.0f;
    }
    return SPCBPT_OK;
}

}  // namespace

extern "C" int spcbpt_denoise_variance_host(const float* accum_rgba, const float* m2n, const float* albedo_rgba, const float* normal_depth_rgba,
                                            const float eye[3], const float U[3], const float V[3], const float W[3],
                                            int width, int height, const spcbpt_denoise_params* p, float* out_rgba) {
    using namespace spc;
    if (!accum_rgba || !m2n || !albedo_rgba || !normal_depth_rgba || !eye || !U || !V || !W || !p || !out_rgba) return SPCBPT_ERR_INVALID_ARG;
    if (width < 1 || height < 1 || (long long)width * height > (1ll << 28)) return SPCBPT_ERR_INVALID_ARG;
    if (p->iterations < 1 || p->iterations > kDenoiseMaxIterations) return SPCBPT_ERR_INVALID_ARG;
    const size_t px = (size_t)width * height;
    std::vector<float> c(px * 3), n(px * 3), X(px * 3), v(px);
    const float diag = host_guides(accum_rgba, albedo_rgba, normal_depth_rgba, U, V, W, width, height, c, n, X);
    for (size_t i = 0; i < px; i++) v[i] = denoise_variance_start(&c[i * 3], albedo_rgba + i * 4, m2n + i * 4);
    return host_variance_filter(c, v, n, X, diag, albedo_rgba, width, height, p, out_rgba);
}

// spcbpt_history_denoise on the host: the same filter from the resolved image and its per-channel variance
extern "C" int spcbpt_history_denoise_host(const float* resolved_rgba, const float* resolved_var, const float* albedo_rgba, const float* normal_depth_rgba,
                                           const float eye[3], const float U[3], const float V[3], const float W[3],
                                           int width, int height, const spcbpt_denoise_params* p, float* out_rgba) {
    using namespace spc;
    if (!resolved_rgba || !resolved_var || !albedo_rgba || !normal_depth_rgba || !eye || !U || !V || !W || !p || !out_rgba) return SPCBPT_ERR_INVALID_ARG;
    if (width < 1 || height < 1 || (long long)width * height > (1ll << 28)) return SPCBPT_ERR_INVALID_ARG;
    if (p->iterations < 1 || p->iterations > kDenoiseMaxIterations) return SPCBPT_ERR_INVALID_ARG;
    const size_t px = (size_t)width * height;
    std::vector<float> c(px * 3), n(px * 3), X(px * 3), v(px);
    const float diag = host_guides(resolved_rgba, albedo_rgba, normal_depth_rgba, U, V, W, width, height, c, n, X);
    for (size_t i = 0; i < px; i++) v[i] = denoise_resolved_start(albedo_rgba + i * 4, resolved_var + i * 4);
    return host_variance_filter(c, v, n, X, diag, albedo_rgba, width, height, p, out_rgba);
}

extern "C" int spcbpt_denoise_host(const float* accum_rgba, const float* albedo_rgba, const float* normal_depth_rgba,
                                   const float eye[3], const float U[3], const float V[3], const float W[3],
                                   int width, int height, const spcbpt_denoise_params* p, float* out_rgba) {
    using namespace spc;
    if (!accum_rgba || !albedo_rgba || !normal_depth_rgba || !eye || !U || !V || !W || !p || !out_rgba) return SPCBPT_ERR_INVALID_ARG;
    if (width < 1 || height < 1 || (long long)width * height > (1ll << 28)) return SPCBPT_ERR_INVALID_ARG;
    if (p->iterations < 1 || p->iterations > kDenoiseMaxIterations) return SPCBPT_ERR_INVALID_ARG;
    // the host has no scene: sigma_x <= 0 takes the default fraction of the extent of the positions themselves
    const size_t px = (size_t)width * height;
    std::vector<float> c(px * 3), c2(px * 3), n(px * 3), X(px * 3);
    const float diag = host_guides(accum_rgba, albedo_rgba, normal_depth_rgba, U, V, W, width, height, c, n, X);
    const float sigma_c = p->sigma_c > 0.0f ? p->sigma_c : SPCBPT_DENOISE_SIGMA_C;
    const float sigma_n = p->sigma_n > 0.0f ? p->sigma_n : SPCBPT_DENOISE_SIGMA_N;
    const float sigma_x = p->sigma_x > 0.0f ? p->sigma_x : SPCBPT_DENOISE_SIGMA_X_FRACTION * (diag > 0.0f ? diag : 1.0f);
    for (int it = 0; it < p->iterations; it++) {
        const AtrousStep a = atrous_step(it, sigma_c, sigma_n, sigma_x);
        const HostPlanes f = {c.data(), n.data(), X.data(), width};
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) atrous_pixel(f, x, y, width, height, a, &c2[((size_t)y * width + x) * 3]);
        c.swap(c2);
    }
    for (size_t i = 0; i < px; i++) {
        denoise_remodulate(&c[i * 3], albedo_rgba + i * 4, out_rgba + i * 4);
        out_rgba[i * 4 + 3] = 1.0f;
    }
    return SPCBPT_OK;
}
