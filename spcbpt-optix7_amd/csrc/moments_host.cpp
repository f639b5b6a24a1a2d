// spcbpt_film_moments_update_host / spcbpt_film_error_host: the film's second moment and its error estimate on caller buffers, on the
// host -- moments_pixel.h, the header the kernels of kernels_moments.hip run, over plain arrays.  No context, no GPU (plain g++,
// -ffp-contract=off like the device code).
#include "../../include/spcbpt.h"
#include "moments_pixel.h"

extern "C" int spcbpt_film_moments_update_host(const float* mean_before_rgba, const float* sample_rgba, uint32_t subframe, int64_t n_pixels,
                                               float* m2n_inout) {
    if (!mean_before_rgba || !sample_rgba || !m2n_inout || n_pixels < 1 || n_pixels > (1ll << 28)) return SPCBPT_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n_pixels; i++) spc::film_moments_update(mean_before_rgba + i * 4, sample_rgba + i * 4, subframe, m2n_inout + i * 4);
    return SPCBPT_OK;
}

extern "C" int spcbpt_film_error_host(const float* accum_rgba, const float* m2n, int64_t n_pixels, spcbpt_film_error_stats* out) {
    if (!accum_rgba || !m2n || !out || n_pixels < 1 || n_pixels > (1ll << 28)) return SPCBPT_ERR_INVALID_ARG;
    double sum = 0.0;
    float top = 0.0f;
    int64_t count = 0;
    for (int64_t i = 0; i < n_pixels; i++) {
        float e;
        if (!spc::film_error_pixel(accum_rgba + i * 4, m2n + i * 4, &e)) continue;
        sum += (double)e;
        top = fmaxf(top, e);
        count++;
    }
    out->pixels = count;
    out->mean = count ? sum / (double)count : 0.0;
    out->max = count ? (double)top : 0.0;
    return SPCBPT_OK;
}
