// spcbpt_display_host: the display transform on caller buffers, on the host -- display_pixel.h, the header the kernels of
// kernels_display.hip run, over plain arrays.  No context, no GPU (plain g++, -ffp-contract=off like the device code).  Also the two
// host-only pieces the context shares with it: the parameter check and the exposure parameters (the pass's one logarithm).
#include "../../include/spcbpt.h"
#include "display_pixel.h"

namespace spc {

const char* display_params_error(int op, uint32_t flags, float ev, float key, float low_fraction, float high_fraction, float ev_bias, float ev_min,
                                 float ev_max, float adapt, float white) {
    const float f[9] = {ev, key, low_fraction, high_fraction, ev_bias, ev_min, ev_max, adapt, white};
    for (float v : f)
        if (!isfinite(v)) return "display: a parameter is not a finite number";
    if (op < 0 || op >= kDisplayOps) return "display: op must be 0 (film), 1 (reinhard), 2 (aces) or 3 (linear)";
    if (flags & ~(uint32_t)(SPCBPT_DISPLAY_AUTO | SPCBPT_DISPLAY_HISTOGRAM)) return "display: unknown flag bits";
    if (!(low_fraction >= 0.0f && low_fraction < 1.0f && high_fraction >= 0.0f && high_fraction < 1.0f) || !((double)low_fraction + (double)high_fraction < 1.0))
        return "display: low_fraction and high_fraction must be in [0, 1) and sum to less than 1";
    if (ev_min > ev_max) return "display: ev_min is above ev_max";
    if (!(adapt > 0.0f && adapt <= 1.0f)) return "display: adapt must be in (0, 1]";
    if (!(key > 0.0f)) return "display: key must be > 0";
    if (!(white > 0.0f)) return "display: white must be > 0";
    return nullptr;
}

DisplayExposure display_exposure_of(float key, float low_fraction, float high_fraction, float ev_bias, float ev_min, float ev_max, float adapt) {
    DisplayExposure q;
    q.log2_key = log2((double)key);
    q.low_fraction = (double)low_fraction; q.high_fraction = (double)high_fraction;
    q.ev_bias = (double)ev_bias; q.ev_min = (double)ev_min; q.ev_max = (double)ev_max; q.adapt = (double)adapt;
    return q;
}

}  // namespace spc

extern "C" int spcbpt_display_default_params(spcbpt_display_params* p) {
    if (!p) return SPCBPT_ERR_INVALID_ARG;
    p->op = SPCBPT_TONE_FILM; p->flags = 0; p->ev = 0.0f; p->key = 0.18f;
    p->low_fraction = 0.05f; p->high_fraction = 0.02f;
    p->ev_bias = 0.0f; p->ev_min = -16.0f; p->ev_max = 16.0f;
    p->adapt = 1.0f; p->white = 4.0f;
    return SPCBPT_OK;
}

extern "C" int spcbpt_display_params_struct_size(void) { return (int)sizeof(spcbpt_display_params); }

extern "C" int spcbpt_display_host(const float* rgba, int64_t n_pixels, const spcbpt_display_params* p, int have_prev, float prev_ev,
                                   uint8_t* rgba8_out, uint32_t* histogram_out, float* ev_out) {
    if (!rgba || !p || n_pixels < 1 || n_pixels > (1ll << 28)) return SPCBPT_ERR_INVALID_ARG;
    if (spc::display_params_error(p->op, p->flags, p->ev, p->key, p->low_fraction, p->high_fraction, p->ev_bias, p->ev_min, p->ev_max, p->adapt, p->white))
        return SPCBPT_ERR_INVALID_ARG;
    const bool auto_ev = (p->flags & SPCBPT_DISPLAY_AUTO) != 0;
    if (auto_ev && have_prev && !isfinite(prev_ev)) return SPCBPT_ERR_INVALID_ARG;
    uint32_t counters[spc::kDisplayCounters] = {0};
    for (int64_t i = 0; i < n_pixels; i++) counters[spc::display_bin(spc::display_luminance(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2]))]++;
    float ev = p->ev;
    if (auto_ev)
        ev = spc::display_auto_ev(counters, spc::display_exposure_of(p->key, p->low_fraction, p->high_fraction, p->ev_bias, p->ev_min, p->ev_max, p->adapt),
                                  have_prev != 0, prev_ev);
    if (histogram_out) memcpy(histogram_out, counters, sizeof(counters));
    if (ev_out) *ev_out = ev;
    if (rgba8_out) {
        const float scale = exp2f(ev);
        for (int64_t i = 0; i < n_pixels; i++) {
            const uint32_t v = spc::display_tone(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2], scale, p->op, p->white);
            memcpy(rgba8_out + 4 * i, &v, 4);
        }
    }
    return SPCBPT_OK;
}
