// spcbpt_bloom_host: the bloom stage on caller buffers, on the host -- bloom_pixel.h, the header the kernels of kernels_bloom.hip run,
// over plain arrays.  No context, no GPU (plain g++, -ffp-contract=off like the device code).  Also the two host-only pieces the
// context shares with it: the parameter check and the plan of the pyramid (level sizes, offsets, level weights).
#include "../../include/spcbpt.h"
#include "bloom_pixel.h"

#include <vector>

namespace spc {

const char* bloom_params_error(int levels, float strength, float spread, float threshold, float clamp) {
    const float f[4] = {strength, spread, threshold, clamp};
    for (float v : f)
        if (!isfinite(v)) return "bloom: a parameter is not a finite number";
    if (levels < 1 || levels > kBloomMaxLevels) return "bloom: levels must be 1 .. 8";
    if (!(strength >= 0.0f && strength <= 1.0f)) return "bloom: strength must be in [0, 1]";
    if (!(spread > 0.0f && spread <= 4.0f)) return "bloom: spread must be in (0, 4]";
    if (!(threshold >= 0.0f)) return "bloom: threshold must be >= 0";
    if (!(clamp > 0.0f && clamp <= 18446744073709551616.0f)) return "bloom: clamp must be in (0, 2^64]";
    return nullptr;
}

BloomPlan bloom_plan_of(int width, int height, int levels, float spread) {
    BloomPlan q;
    q.levels = levels;
    q.w[0] = width; q.h[0] = height; q.off[0] = 0; q.g[0] = 0.0f;
    size_t at = 0;
    for (int k = 1; k <= kBloomMaxLevels; k++) {
        q.w[k] = (q.w[k - 1] + 1) / 2; q.h[k] = (q.h[k - 1] + 1) / 2;
        q.off[k] = at;
        if (k <= levels) at += (size_t)q.w[k] * q.h[k];
        q.g[k] = 0.0f;
    }
    q.texels = at;
    double sum = 0.0, pw = 1.0;
    for (int k = 1; k <= levels; k++) { sum += pw; pw *= (double)spread; }
    pw = 1.0;
    for (int k = 1; k <= levels; k++) { q.g[k] = (float)(pw / sum); pw *= (double)spread; }
    return q;
}

namespace {

struct HostAt {   // a level as a plain array of BloomPx, clamped addressing
    const BloomPx* p;
    int w, h;
    BloomPx operator()(int x, int y) const { return p[(size_t)bloom_clampi(y, h - 1) * w + bloom_clampi(x, w - 1)]; }
};

}  // namespace

}  // namespace spc

extern "C" int spcbpt_bloom_default_params(spcbpt_bloom_params* p) {
    if (!p) return SPCBPT_ERR_INVALID_ARG;
    p->levels = 5; p->strength = 0.1f; p->spread = 1.0f; p->threshold = 0.0f; p->clamp = 65504.0f;
    return SPCBPT_OK;
}

extern "C" int spcbpt_bloom_params_struct_size(void) { return (int)sizeof(spcbpt_bloom_params); }

extern "C" int spcbpt_bloom_host(const float* rgba, int width, int height, const spcbpt_bloom_params* p, float* out_rgba) {
    using namespace spc;
    if (!rgba || !p || !out_rgba || width < 1 || height < 1 || (int64_t)width * height > (1ll << 28)) return SPCBPT_ERR_INVALID_ARG;
    if (bloom_params_error(p->levels, p->strength, p->spread, p->threshold, p->clamp)) return SPCBPT_ERR_INVALID_ARG;
    const BloomPlan q = bloom_plan_of(width, height, p->levels, p->spread);
    const int L = q.levels;
    const size_t px = (size_t)width * height;
    std::vector<BloomPx> P(px), pyr(q.texels);
    for (size_t i = 0; i < px; i++) P[i] = bloom_pre(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], p->threshold, p->clamp);
    // down: D_k from D_{k-1}; the coarsest level is stored as U_L = g_L D_L
    for (int k = 1; k <= L; k++) {
        const HostAt src{k == 1 ? P.data() : pyr.data() + q.off[k - 1], q.w[k - 1], q.h[k - 1]};
        BloomPx* dst = pyr.data() + q.off[k];
        for (int y = 0; y < q.h[k]; y++)
            for (int x = 0; x < q.w[k]; x++) {
                const BloomPx d = bloom_down(src, x, y);
                dst[(size_t)y * q.w[k] + x] = k == L ? bloom_scale(q.g[L], d) : d;
            }
    }
    // up and mix, in place: U_k = g_k D_k + up(U_{k+1})
    for (int k = L - 1; k >= 1; k--) {
        const HostAt coarse{pyr.data() + q.off[k + 1], q.w[k + 1], q.h[k + 1]};
        BloomPx* dst = pyr.data() + q.off[k];
        for (int y = 0; y < q.h[k]; y++)
            for (int x = 0; x < q.w[k]; x++) {
                BloomPx& d = dst[(size_t)y * q.w[k] + x];
                d = bloom_mix(q.g[k], d, bloom_up(coarse, x, y));
            }
    }
    // composite: O = I + s (up(U_1) - P)
    const HostAt u1{pyr.data() + q.off[1], q.w[1], q.h[1]};
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const size_t i = (size_t)y * width + x;
            const BloomPx B = bloom_up(u1, x, y);
            out_rgba[4 * i] = bloom_composite(rgba[4 * i], p->strength, B.r, P[i].r);
            out_rgba[4 * i + 1] = bloom_composite(rgba[4 * i + 1], p->strength, B.g, P[i].g);
            out_rgba[4 * i + 2] = bloom_composite(rgba[4 * i + 2], p->strength, B.b, P[i].b);
            out_rgba[4 * i + 3] = rgba[4 * i + 3];
        }
    return SPCBPT_OK;
}
