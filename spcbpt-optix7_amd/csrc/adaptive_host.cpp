// spcbpt_adaptive_select_host: the tile errors and the tile list of adaptive sampling on caller buffers, on the host --
// adaptive_pixel.h, the header the kernels of kernels_adaptive.hip run, over plain arrays.  No context, no GPU (plain g++,
// -ffp-contract=off like the device code).
#include "../../include/spcbpt.h"
#include "adaptive_pixel.h"

extern "C" int spcbpt_adaptive_params_struct_size(void) { return (int)sizeof(spcbpt_adaptive_params); }

extern "C" int spcbpt_adaptive_select_host(const float* accum_rgba, const float* m2n, int width, int height, const uint32_t* tile_samples,
                                           const spcbpt_adaptive_params* params, float* tile_error_out, uint32_t* tiles_out, int* n_out) {
    if (!accum_rgba || !m2n || !tile_samples || !params || width < 1 || height < 1 || (long long)width * height > (1ll << 28)) return SPCBPT_ERR_INVALID_ARG;
    if (!(params->target_error == params->target_error)) return SPCBPT_ERR_INVALID_ARG;
    const uint32_t w = (uint32_t)width, h = (uint32_t)height;
    const uint32_t n_tiles = spc::adaptive_tiles_x(w) * spc::adaptive_tiles_y(h);
    int n = 0;
    for (uint32_t t = 0; t < n_tiles; t++) {
        float e[64];
        uint32_t have[64];
        for (uint32_t s = 0; s < 64; s++) {
            uint32_t x, y;
            const bool inside = spc::adaptive_tile_pixel(w, h, t, s, &x, &y);
            const size_t idx = inside ? (size_t)y * w + x : 0;
            spc::adaptive_slot_term(accum_rgba + idx * 4, m2n + idx * 4, inside, &e[s], &have[s]);
        }
        for (uint32_t off = 32; off > 0; off >>= 1)
            for (uint32_t s = 0; s < off; s++) { e[s] += e[s + off]; have[s] += have[s + off]; }
        const float e_t = spc::adaptive_tile_mean(e[0], have[0]);
        if (tile_error_out) tile_error_out[t] = e_t;
        if (spc::adaptive_tile_selected(tile_samples[t], e_t, have[0] == 0u, params->target_error, params->min_samples, params->max_samples)) {
            if (tiles_out) tiles_out[n] = t;
            n++;
        }
    }
    if (n_out) *n_out = n;
    return SPCBPT_OK;
}
