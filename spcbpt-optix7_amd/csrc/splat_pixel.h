// The per-pixel work of the ordered mode of "lt" (spcbpt_set_splat_order): a pixel's radiance as the sum of its splat records in
// ascending cache order, one float32 addition per record and channel.  One set of __host__ __device__ functions shared by
// k_lt_gather (kernels_splat.hip) and the exported spcbpt_splat_sum_host (splat_host.cpp, plain g++), so that the order -- the
// only thing the mode is about -- is testable without a GPU.  Float32 throughout, no contraction (the library's flags; there is no
// multiplication here to fuse).  Includes no device header (the moments_pixel.h pattern).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SPC_SP_HD __host__ __device__ inline
#else
#define SPC_SP_HD inline
#endif

#include <stdint.h>

namespace spc {

// acc += rgb: THE addition of the definition.  A sum starts from +0.0f, so a pixel without a record is +0.0f.
SPC_SP_HD void splat_add(float* acc, const float* rgb) {
    acc[0] = acc[0] + rgb[0];
    acc[1] = acc[1] + rgb[1];
    acc[2] = acc[2] + rgb[2];
}

// first j in [0, n) with keys[j] >= key (n if none); keys ascending
SPC_SP_HD uint32_t splat_lower_bound(const uint32_t* keys, uint32_t n, uint32_t key) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The segment of `key` in a stably sorted (key, vertex index) list of n items: keys ascending, and within one key the vertex indices
// `order` in ascending order (what a stable sort of the pairs (key_i, i) leaves).  records: `stride` floats per vertex, rgb first.
// acc = +0 + rgb[order[a]] + rgb[order[a + 1]] + ... in that order; returns the number of records added.
SPC_SP_HD uint32_t splat_segment_sum(const uint32_t* keys, const uint32_t* order, uint32_t n, uint32_t key, const float* records, int stride,
                                     float* acc) {
    acc[0] = acc[1] = acc[2] = 0.0f;
    uint32_t j = splat_lower_bound(keys, n, key);
    const uint32_t first = j;
    for (; j < n && keys[j] == key; j++) splat_add(acc, records + (size_t)order[j] * (size_t)stride);
    return j - first;
}

}  // namespace spc
