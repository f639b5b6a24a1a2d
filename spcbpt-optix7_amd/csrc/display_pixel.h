// The per-pixel work of the display transform -- luminance histogram, auto exposure, tone operators -- as one set of __host__
// __device__ functions shared by k_display_histogram / k_display_exposure / k_display_map (kernels_display.hip) and the exported
// spcbpt_display_host (display_host.cpp, plain g++), so that all of it is testable without a GPU.  Float32 per pixel, double in the
// exposure, no contraction (the library's flags), the same operations in the same order on both sides.  Includes no device header
// (the moments_pixel.h pattern).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SPC_DP_HD __host__ __device__ inline
#else
#define SPC_DP_HD inline
#endif

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace spc {

// ---- histogram: 256 bins over the 32 octaves [2^-16, 2^16), eight per octave, cut from the float's bit pattern (exponent and the top
// three mantissa bits), so that host and device agree bin for bin without a logarithm; then `dark` (everything that is not >= 2^-16:
// zero, negatives, NaN) and `bright` (everything >= 2^16, +inf included).  The 258 counters sum to the pixel count.
static constexpr int kDisplayBins = 256, kDisplayDark = 256, kDisplayBright = 257, kDisplayCounters = 258;
static constexpr int kDisplayOctaveLo = -16, kDisplayOctaves = 32;
static constexpr int kDisplayOps = 4;   // 0 FILM, 1 REINHARD, 2 ACES, 3 LINEAR

SPC_DP_HD float display_luminance(float r, float g, float b) { return 0.3f * r + 0.6f * g + 0.1f * b; }   // the project's weights, in film_write's order

SPC_DP_HD int display_bin(float L) {
    if (!(L >= 1.52587890625e-05f)) return kDisplayDark;   // 2^-16
    if (L >= 65536.0f) return kDisplayBright;              // 2^16
    uint32_t u;
    memcpy(&u, &L, 4);
    return (int)(u >> 20) - ((127 + kDisplayOctaveLo) << 3);
}

// The parameters of the exposure as the kernel takes them: spcbpt_display_params' fields in double, with log2(key) taken ON THE HOST
// (by the context and by spcbpt_display_host alike), so that only + - x / are left on the path and the IEEE device build returns the
// host's bits.
struct DisplayExposure {
    double log2_key, low_fraction, high_fraction, ev_bias, ev_min, ev_max, adapt;
};

// Host only, defined once (display_host.cpp) for the context and for spcbpt_display_host: NULL, or what is wrong with the fields of
// a spcbpt_display_params; and the exposure parameters of valid ones (the one log2 of the pass).
const char* display_params_error(int op, uint32_t flags, float ev, float key, float low_fraction, float high_fraction, float ev_bias, float ev_min,
                                 float ev_max, float adapt, float white);
DisplayExposure display_exposure_of(float key, float low_fraction, float high_fraction, float ev_bias, float ev_min, float ev_max, float adapt);

SPC_DP_HD double display_clamp_ev(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// EV from the 258 counters.  Over the in-range bins (N samples in ascending luminance): the lowest (uint64)(low_fraction N) and the
// highest (uint64)(high_fraction N) samples are dropped -- a bin may be cut partially --, mean = the count-weighted mean of the kept
// bins' centres in log2, e + log2(1 + (m + 0.5) / 8) for octave e and sub-bin m (the eight logarithms are literals), summed in
// ascending bin order.   target = clamp(log2(key) - mean + ev_bias, ev_min, ev_max);   EV = prev + adapt (target - prev) with a
// previous EV, else target.   No in-range pixel: EV = prev, or clamp(ev_bias) without one.
SPC_DP_HD float display_auto_ev(const uint32_t* counters, const DisplayExposure& q, bool have_prev, float prev_ev) {
    const double centre[8] = {0.087462841250339401, 0.24792751344358549, 0.39231742277876031, 0.52356195605701283,
                              0.6438561897747247,   0.75488750216346856, 0.85798099512757209, 0.95419631038687525};
    // (both walks go octave by octave with the eight sub-bins unrolled: on the device the eight counters of an octave are then one
    // wide load, where a loop over 256 bins waits for 256 loads one after the other)
    uint64_t N = 0;
    for (int o = 0; o < kDisplayOctaves; o++) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int m = 0; m < 8; m++) N += counters[8 * o + m];
    }
    if (N == 0) return have_prev ? prev_ev : (float)display_clamp_ev(q.ev_bias, q.ev_min, q.ev_max);
    const uint64_t lo = (uint64_t)(q.low_fraction * (double)N);
    const uint64_t hi = N - (uint64_t)(q.high_fraction * (double)N);   // the kept samples are [lo, hi) of the N in ascending order
    double sum = 0.0;
    uint64_t start = 0, kept_total = 0;
    for (int o = 0; o < kDisplayOctaves; o++) {
        uint32_t c[8];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int m = 0; m < 8; m++) c[m] = counters[8 * o + m];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int m = 0; m < 8; m++) {
            const uint64_t end = start + c[m];
            const uint64_t a = start > lo ? start : lo, z = end < hi ? end : hi;
            if (z > a) {
                const uint64_t kept = z - a;
                sum = sum + (double)kept * ((double)(o + kDisplayOctaveLo) + centre[m]);
                kept_total += kept;
            }
            start = end;
        }
    }
    if (kept_total == 0) return have_prev ? prev_ev : (float)display_clamp_ev(q.ev_bias, q.ev_min, q.ev_max);   // (fractions summing to < 1 keep >= 1 sample)
    const double mean = sum / (double)kept_total;
    const double target = display_clamp_ev(q.log2_key - mean + q.ev_bias, q.ev_min, q.ev_max);
    if (!have_prev) return (float)target;
    const double prev = (double)prev_ev;
    return (float)(prev + q.adapt * (target - prev));
}

// ---- tone operators on c' = c scale, scale = 2^EV; then clamp, sRGB, 8 bits, alpha 255.  The tail is film_tone_map's (device_lib.h)
// operation for operation, and so is operator 0 as a whole: at EV 0 (scale exactly 1) the device returns the frame's bytes.
SPC_DP_HD float display_to_srgb(float c) { return c < 0.0031308f ? 12.92f * c : 1.055f * powf(c, 1.0f / 2.4f) - 0.055f; }
SPC_DP_HD float display_clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
SPC_DP_HD uint32_t display_quant8(float x) {
    x = display_clamp01(x);
    const uint32_t q = (uint32_t)(x * 256.0f);
    return q < 255u ? q : 255u;
}

SPC_DP_HD uint32_t display_tone(float r, float g, float b, float scale, int op, float white) {
    float c[3] = {r * scale, g * scale, b * scale};
    if (op == 0) {          // FILM: c / (1 + lum / 1.5)
        const float lum = display_luminance(c[0], c[1], c[2]);
        const float s = 1.0f / (1.0f + lum / 1.5f);
        for (int k = 0; k < 3; k++) c[k] = c[k] * s;
    } else if (op == 1) {   // REINHARD (extended): c (1 + L / white^2) / (1 + L)
        const float lum = display_luminance(c[0], c[1], c[2]);
        const float s = (1.0f + lum / (white * white)) / (1.0f + lum);
        for (int k = 0; k < 3; k++) c[k] = c[k] * s;
    } else if (op == 2) {   // ACES, the fitted curve, per channel
        for (int k = 0; k < 3; k++) {
            const float x = c[k];
            c[k] = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
        }
    }                       // 3 LINEAR: c' itself
    return display_quant8(display_to_srgb(display_clamp01(c[0]))) | (display_quant8(display_to_srgb(display_clamp01(c[1]))) << 8) |
           (display_quant8(display_to_srgb(display_clamp01(c[2]))) << 16) | (255u << 24);
}

}  // namespace spc
