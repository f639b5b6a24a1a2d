// The per-tile work of adaptive sampling: one set of __host__ __device__ functions shared by k_tile_error / k_tile_select
// (kernels_adaptive.hip) and the exported spcbpt_adaptive_select_host (adaptive_host.cpp, plain g++), so that both are testable
// without a GPU.  Float32 throughout, no contraction (the library's flags), the same operations in the same order on both sides.
// Includes no device header (the moments_pixel.h pattern).
#pragma once
#include "moments_pixel.h"

namespace spc {

// A tile is an 8x8 pixel block of the whole film, numbered x-major: tile_pixel's numbering (eye_walk.h) with row_begin = 0,
// row_step = 1.  Edge tiles are partial.
SPC_MO_HD uint32_t adaptive_tiles_x(uint32_t width) { return (width + 7u) / 8u; }
SPC_MO_HD uint32_t adaptive_tiles_y(uint32_t height) { return (height + 7u) / 8u; }
// pixel of slot 0 .. 63 of tile t; false outside the image
SPC_MO_HD bool adaptive_tile_pixel(uint32_t width, uint32_t height, uint32_t tile, uint32_t slot, uint32_t* x, uint32_t* y) {
    const uint32_t tiles_x = adaptive_tiles_x(width);
    *x = (tile % tiles_x) * 8u + (slot & 7u);
    *y = (tile / tiles_x) * 8u + (slot >> 3);
    return *x < width && *y < height;
}

// Slot s of a tile contributes (e, 1) if its pixel is inside the image and has n >= 2 (film_error_pixel), (0, 0) otherwise.
SPC_MO_HD void adaptive_slot_term(const float* accum, const float* m2n, bool inside, float* e, uint32_t* have) {
    float v = 0.0f;
    const bool ok = inside && film_error_pixel(accum, m2n, &v);
    *e = ok ? v : 0.0f;
    *have = ok ? 1u : 0u;
}
// The 64 slot terms are added by halving: round off = 32, 16, ..., 1 adds slot s + off to slot s for s < off.  That is what a wave's
// __shfl_down tree leaves in lane 0, so the host walks the same tree over an array.  e_t = sum / count; no pixel with n >= 2: e_t = 0
// and the tile is "unknown".
SPC_MO_HD float adaptive_tile_mean(float sum, uint32_t count) { return count ? sum / (float)count : 0.0f; }

// A tile is traced again iff it is below the sample cap AND (it has fewer than max(min_samples, 2) samples, OR nothing is known
// about it, OR its error is above the target).
SPC_MO_HD bool adaptive_tile_selected(uint32_t samples, float e, bool unknown, float target_error, uint32_t min_samples, uint32_t max_samples) {
    if (max_samples != 0u && samples >= max_samples) return false;
    const uint32_t floor_n = min_samples > 2u ? min_samples : 2u;
    return samples < floor_n || unknown || e > target_error;
}

}  // namespace spc
