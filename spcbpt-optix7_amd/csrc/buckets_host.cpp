// spcbpt_film_buckets_update_host / spcbpt_robust_resolve_host: the bucket film and its median-of-means resolve on caller buffers, on
// the host -- buckets_pixel.h, the header the kernels of kernels_buckets.hip run, over plain arrays.  No context, no GPU (plain g++,
// -ffp-contract=off like the device code).
#include "../../include/spcbpt.h"
#include "buckets_pixel.h"

static bool bad_count(int64_t n_pixels) { return n_pixels < 1 || n_pixels > (1ll << 28); }

extern "C" int spcbpt_film_buckets_update_host(const float* sample_rgba, uint32_t subframe, int buckets, int64_t n_pixels, float* planes_inout) {
    if (!sample_rgba || !planes_inout || !spc::film_buckets_valid(buckets) || bad_count(n_pixels)) return SPCBPT_ERR_INVALID_ARG;
    const int64_t b = (int64_t)(subframe % (uint32_t)buckets);
    for (int64_t i = 0; i < n_pixels; i++) {
        if (subframe == 0)
            for (int64_t k = 0; k < buckets; k++)
                for (int c = 0; c < 4; c++) planes_inout[(k * n_pixels + i) * 4 + c] = 0.0f;
        spc::film_bucket_update(sample_rgba + i * 4, planes_inout + (b * n_pixels + i) * 4);
    }
    return SPCBPT_OK;
}

extern "C" int spcbpt_robust_resolve_host(const float* planes, int buckets, int64_t n_pixels, float strength, float* out_rgba) {
    if (!planes || !out_rgba || !spc::film_buckets_valid(buckets) || bad_count(n_pixels)) return SPCBPT_ERR_INVALID_ARG;
    if (!(strength >= 0.0f && strength <= 8.0f)) return SPCBPT_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n_pixels; i++) {
        float bk[spc::kBucketsMax][4];
        for (int64_t k = 0; k < buckets; k++)
            for (int c = 0; c < 4; c++) bk[k][c] = planes[(k * n_pixels + i) * 4 + c];
        spc::robust_resolve_pixel<spc::kBucketsMax>(bk, buckets, strength, out_rgba + i * 4);
    }
    return SPCBPT_OK;
}
