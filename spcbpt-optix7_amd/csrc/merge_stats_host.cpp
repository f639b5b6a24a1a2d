// spcbpt_film_merge_batch_host: the batched film merge with moments and buckets on caller buffers, on the host -- merge_stats_pixel.h,
// the header k_film_merge_batch_stats (kernels_merge_stats.hip) runs, over plain arrays.  No context, no GPU (plain g++,
// -ffp-contract=off like the device code).
#include "../../include/spcbpt.h"
#include "merge_stats_pixel.h"

namespace {

struct PlaneEntry {   // pixel i of the caller's [K][n_pixels][4] planes
    float* planes;
    int64_t n_pixels, i;
    void load(int b, float* m) const { for (int c = 0; c < 4; c++) m[c] = planes[((int64_t)b * n_pixels + i) * 4 + c]; }
    void store(int b, const float* m) const { for (int c = 0; c < 4; c++) planes[((int64_t)b * n_pixels + i) * 4 + c] = m[c]; }
};

template <bool MOMENTS, bool BUCKETS>
void run(const float* samples, const uint32_t* subframes, int n, int64_t n_pixels, int buckets, float* accum, float* m2n, float* planes) {
    for (int64_t i = 0; i < n_pixels; i++) {
        float c[3] = {accum[i * 4], accum[i * 4 + 1], accum[i * 4 + 2]};
        float none[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        spc::film_merge_stats_pixel<MOMENTS, BUCKETS>(
            n, subframes,
            [&](int k, float* x) { const float* s = samples + ((int64_t)k * n_pixels + i) * 4; x[0] = s[0]; x[1] = s[1]; x[2] = s[2]; },
            buckets, PlaneEntry{planes, n_pixels, i}, c, MOMENTS ? m2n + i * 4 : none);
        accum[i * 4] = c[0]; accum[i * 4 + 1] = c[1]; accum[i * 4 + 2] = c[2]; accum[i * 4 + 3] = 1.0f;   // the film's alpha
    }
}

}  // namespace

extern "C" int spcbpt_film_merge_batch_host(const float* samples, const uint32_t* subframes, int n, int64_t n_pixels, int buckets,
                                            float* accum_inout, float* m2n_inout_or_null, float* planes_inout_or_null) {
    if (!samples || !subframes || !accum_inout || n < 1 || n > spc::kMergeStatsMaxFrames || n_pixels < 1 || n_pixels > (1ll << 28)) return SPCBPT_ERR_INVALID_ARG;
    if (buckets != 0 && (!spc::film_buckets_valid(buckets) || !planes_inout_or_null)) return SPCBPT_ERR_INVALID_ARG;
    const bool mo = m2n_inout_or_null != nullptr, bk = buckets != 0;
    if (mo && bk) run<true, true>(samples, subframes, n, n_pixels, buckets, accum_inout, m2n_inout_or_null, planes_inout_or_null);
    else if (mo) run<true, false>(samples, subframes, n, n_pixels, buckets, accum_inout, m2n_inout_or_null, nullptr);
    else if (bk) run<false, true>(samples, subframes, n, n_pixels, buckets, accum_inout, nullptr, planes_inout_or_null);
    else run<false, false>(samples, subframes, n, n_pixels, buckets, accum_inout, nullptr, nullptr);
    return SPCBPT_OK;
}
