// spcbpt_history_reproject_host / spcbpt_history_resolve_host (and their variance-carrying _var_ forms): the passes of spcbpt_history_reproject / spcbpt_history_resolve on
// caller buffers, on the host -- reproject_pixel.h, the header the kernels of kernels_reproject.hip run, over plain arrays.  No
// context, no GPU (plain g++, -ffp-contract=off like the device code).
#include <cstring>

#include "../../include/spcbpt.h"
#include "reproject_pixel.h"

namespace {

struct HostHistory {   // reproject_pixel's F over the two history planes, 4 floats per pixel each
    const float *g, *h;
    int width;
    void fetch(int x, int y, float* G, float* H) const {
        const size_t i = ((size_t)y * width + x) * 4;
        for (int k = 0; k < 4; k++) { G[k] = g[i + k]; H[k] = h[i + k]; }
    }
};

struct HostHistoryVar {   // reproject_var_pixel's F: the variance plane beside them
    const float *g, *h, *hv;
    int width;
    void fetch(int x, int y, float* G, float* H, float* HV) const {
        const size_t i = ((size_t)y * width + x) * 4;
        for (int k = 0; k < 4; k++) { G[k] = g[i + k]; H[k] = h[i + k]; HV[k] = hv[i + k]; }
    }
};

spc::ReprojectCamera host_camera(const float* eye, const float* U, const float* V, const float* W) {
    spc::ReprojectCamera c;
    memcpy(c.eye, eye, 12); memcpy(c.U, U, 12); memcpy(c.V, V, 12); memcpy(c.W, W, 12);
    return c;
}

}  // namespace

extern "C" int spcbpt_history_reproject_host(const float eye[3], const float U[3], const float V[3], const float W[3], const float* normal_depth_rgba,
                                             const float eye_h[3], const float U_h[3], const float V_h[3], const float W_h[3],
                                             const float* history_normal_depth_rgba, const float* history_rgbn, int width, int height,
                                             const spcbpt_reproject_params* p, float sigma_x_default_diag, float* prior_out) {
    using namespace spc;
    if (!eye || !U || !V || !W || !normal_depth_rgba || !eye_h || !U_h || !V_h || !W_h || !history_normal_depth_rgba || !history_rgbn || !p || !prior_out) return SPCBPT_ERR_INVALID_ARG;
    if (width < 1 || height < 1 || (long long)width * height > (1ll << 28)) return SPCBPT_ERR_INVALID_ARG;
    if (!(p->sigma_n == p->sigma_n) || !(p->sigma_x == p->sigma_x) || !(p->max_history == p->max_history)) return SPCBPT_ERR_INVALID_ARG;
    const float sigma_n = p->sigma_n > 0.0f ? p->sigma_n : SPCBPT_REPROJECT_SIGMA_N;
    const float sigma_x = p->sigma_x > 0.0f ? p->sigma_x : SPCBPT_REPROJECT_SIGMA_X_FRACTION * (sigma_x_default_diag > 0.0f ? sigma_x_default_diag : 1.0f);
    const float max_history = p->max_history > 0.0f ? p->max_history : SPCBPT_REPROJECT_MAX_HISTORY;
    const ReprojectStep step = reproject_step(sigma_n, sigma_x, max_history);
    const ReprojectCamera cur = host_camera(eye, U, V, W), hist = host_camera(eye_h, U_h, V_h, W_h);
    const HostHistory f = {history_normal_depth_rgba, history_rgbn, width};
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const size_t i = ((size_t)y * width + x) * 4;
            reproject_pixel(f, cur, hist, width, height, x, y, normal_depth_rgba + i, step, prior_out + i);
        }
    return SPCBPT_OK;
}

extern "C" int spcbpt_history_resolve_host(const float* prior_rgba, const float* accum_rgba, uint32_t frames, int64_t n_pixels, float* out_rgba) {
    if (!accum_rgba || !out_rgba || frames == 0 || n_pixels < 1 || n_pixels > (1ll << 28)) return SPCBPT_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n_pixels; i++) spc::resolve_pixel(prior_rgba ? prior_rgba + i * 4 : nullptr, accum_rgba + i * 4, (float)frames, out_rgba + i * 4);
    return SPCBPT_OK;
}

// ---- the variance-carrying forms (spcbpt_history_denoise) ----
extern "C" int spcbpt_history_reproject_var_host(const float eye[3], const float U[3], const float V[3], const float W[3], const float* normal_depth_rgba,
                                                 const float eye_h[3], const float U_h[3], const float V_h[3], const float W_h[3],
                                                 const float* history_normal_depth_rgba, const float* history_rgbn, const float* history_var,
                                                 int width, int height, const spcbpt_reproject_params* p, float sigma_x_default_diag,
                                                 float* prior_out, float* prior_var_out) {
    using namespace spc;
    if (!eye || !U || !V || !W || !normal_depth_rgba || !eye_h || !U_h || !V_h || !W_h || !history_normal_depth_rgba || !history_rgbn || !history_var || !p || !prior_out || !prior_var_out) return SPCBPT_ERR_INVALID_ARG;
    if (width < 1 || height < 1 || (long long)width * height > (1ll << 28)) return SPCBPT_ERR_INVALID_ARG;
    if (!(p->sigma_n == p->sigma_n) || !(p->sigma_x == p->sigma_x) || !(p->max_history == p->max_history)) return SPCBPT_ERR_INVALID_ARG;
    const float sigma_n = p->sigma_n > 0.0f ? p->sigma_n : SPCBPT_REPROJECT_SIGMA_N;
    const float sigma_x = p->sigma_x > 0.0f ? p->sigma_x : SPCBPT_REPROJECT_SIGMA_X_FRACTION * (sigma_x_default_diag > 0.0f ? sigma_x_default_diag : 1.0f);
    const float max_history = p->max_history > 0.0f ? p->max_history : SPCBPT_REPROJECT_MAX_HISTORY;
    const ReprojectStep step = reproject_step(sigma_n, sigma_x, max_history);
    const ReprojectCamera cur = host_camera(eye, U, V, W), hist = host_camera(eye_h, U_h, V_h, W_h);
    const HostHistoryVar f = {history_normal_depth_rgba, history_rgbn, history_var, width};
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const size_t i = ((size_t)y * width + x) * 4;
            reproject_var_pixel(f, cur, hist, width, height, x, y, normal_depth_rgba + i, step, prior_out + i, prior_var_out + i);
        }
    return SPCBPT_OK;
}

extern "C" int spcbpt_history_resolve_var_host(const float* prior_rgba, const float* prior_var, const float* accum_rgba, const float* m2n, uint32_t frames,
                                               int64_t n_pixels, float* out_rgba, float* out_var) {
    if (!accum_rgba || !m2n || !out_rgba || !out_var || (prior_rgba == nullptr) != (prior_var == nullptr)) return SPCBPT_ERR_INVALID_ARG;
    if (frames == 0 || n_pixels < 1 || n_pixels > (1ll << 28)) return SPCBPT_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n_pixels; i++)
        spc::resolve_var_pixel(prior_rgba ? prior_rgba + i * 4 : nullptr, prior_rgba ? prior_var + i * 4 : nullptr, accum_rgba + i * 4, m2n + i * 4, (float)frames,
                               out_rgba + i * 4, out_var + i * 4);
    return SPCBPT_OK;
}
