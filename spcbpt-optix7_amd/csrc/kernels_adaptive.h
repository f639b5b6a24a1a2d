// Launchers of adaptive sampling: the tile errors and the tile list (kernels_adaptive.hip: k_tile_error, k_tile_select), the eye
// megakernel fed from the list (kernels.hip: k_spcbpt_tiles) and the merge of the listed tiles (kernels_adaptive.hip:
// k_film_merge_tiles).  Declared here and not in kernels.h, which is part of the eye megakernel's source hash (source_hash.py).
#pragma once
#include <hip/hip_runtime.h>

#include "adaptive_pixel.h"
#include "layout.h"

namespace spc {

// k_tile_error: one wave per tile, one lane per pixel.  tile_error[t] = e_t, tile_known[t] = the number of its pixels with n >= 2.
void launch_tile_error(const float* accum, const float* m2n, uint32_t width, uint32_t height, float* tile_error, uint32_t* tile_known, hipStream_t s);
// k_tile_select: ONE block compacts the selected tiles into `tiles` in ascending order and leaves their number in *n_out.  No atomics.
void launch_tile_select(const float* tile_error, const uint32_t* tile_known, const uint32_t* tile_samples, uint32_t n_tiles, float target_error,
                        uint32_t min_samples, uint32_t max_samples, uint32_t* tiles, uint32_t* n_out, hipStream_t s);

// The eye megakernel over p.tile_list[0 .. p.n_tiles): its grid (what the spill area is sized for), its occupancy, its launch.
int spcbpt_tiles_blocks(const KParams& p, int max_blocks);
int spcbpt_tiles_blocks_per_cu(bool general);
void launch_spcbpt_tiles(const KParams& p, int max_blocks, hipStream_t s);

struct MergeTilesParams {  // passed by value as the kernel argument block of k_film_merge_tiles
    uint32_t width, height, n_listed;
    const uint32_t* tile_list;   // n_listed tiles, strictly ascending
    uint32_t* tile_samples;      // per tile of the film: read by the tile's wave, then incremented by its lane 0
    const float* result;         // the launch's samples (read only)
    float* accum;
    float* m2n;
    uint32_t* frame;
};
void launch_film_merge_tiles(const MergeTilesParams& p, hipStream_t s);

}  // namespace spc
