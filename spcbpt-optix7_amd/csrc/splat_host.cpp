// spcbpt_splat_sum_host: the ordered splat sum of "lt" on caller buffers, on the host -- splat_pixel.h, the header k_lt_gather
// (kernels_splat.hip) runs, over plain arrays.  No context, no GPU (plain g++, -ffp-contract=off like the device code).
#include "../../include/spcbpt.h"
#include "splat_pixel.h"

extern "C" int spcbpt_splat_sum_host(const float* rgb, const int32_t* pixel, int64_t n, int width, int height, float* out_rgb) {
    if (!out_rgb || n < 0 || (n > 0 && (!rgb || !pixel)) || width < 1 || height < 1 || (int64_t)width * height > (1ll << 28)) return SPCBPT_ERR_INVALID_ARG;
    const int64_t pixels = (int64_t)width * height;
    for (int64_t p = 0; p < pixels * 3; p++) out_rgb[p] = 0.0f;
    // records in ascending index: every pixel's sum takes its own records in ascending index, one addition each
    for (int64_t i = 0; i < n; i++) {
        const int64_t p = pixel[i];
        if (p < 0 || p >= pixels) continue;
        spc::splat_add(out_rgb + p * 3, rgb + i * 3);
    }
    return SPCBPT_OK;
}
