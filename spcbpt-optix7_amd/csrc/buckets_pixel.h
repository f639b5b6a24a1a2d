// The per-pixel work of the bucket film and of its median-of-means resolve: one set of __host__ __device__ functions shared by
// k_film_buckets / k_robust_resolve (kernels_buckets.hip) and the exported spcbpt_film_buckets_update_host /
// spcbpt_robust_resolve_host (buckets_host.cpp, plain g++), so that both are testable without a GPU.  Float32 throughout, no
// contraction (the library's flags), the same operations in the same order on both sides.  Includes no device header (the
// moments_pixel.h pattern).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SPC_BK_HD __host__ __device__ inline
#else
#define SPC_BK_HD inline
#endif

#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace spc {

static constexpr int kBucketsMin = 3, kBucketsMax = 32;
SPC_BK_HD bool film_buckets_valid(int k) { return k >= kBucketsMin && k <= kBucketsMax; }

// One merge of one pixel into its bucket b = subframe % K: bucket = (mean_r, mean_g, mean_b, n) of the samples the bucket has taken,
// `x` the frame's sample.   n' = n + 1,  a = 1 / n',  mean' = mean + a (x - mean)  per channel.
// (The restart of subframe 0 -- every bucket of the pixel to zero first -- is the caller's: it touches all K planes.)
SPC_BK_HD void film_bucket_update(const float* x, float* bucket) {
    const float n = bucket[3] + 1.0f;
    const float a = 1.0f / n;
    for (int c = 0; c < 3; c++) bucket[c] = bucket[c] + a * (x[c] - bucket[c]);
    bucket[3] = n;
}

// The resolve of one pixel from its K buckets, bk[i] = (mean_r, mean_g, mean_b, n_i), i < K <= KP (KP: the compile-time bound the
// loops are unrolled over; entries K .. KP - 1 of bk are never read).  Every sum runs over the buckets in ascending index:
//   live: n_i > 0, k of them (k == 0: out = 0);   y_i = 0.3 r_i + 0.6 g_i + 0.1 b_i
//   rank_i = #{live j: y_j < y_i, or y_j == y_i and j < i}
//   T = sum y_i,   N = sum (float)(2 rank_i - k + 1) y_i
//   G = 0 if k < 3 or !(T > 0), else N / ((float)k T) clamped to [0, 1]             (the Gini coefficient of the bucket luminances)
//   t = ((strength G) (float)k) 0.5,   d = min((k - 1) / 2, (int)floorf(t))
//   kept: d <= rank_i < k - d;   rgb = sum n_i mean_i / sum n_i over the kept,   w = (float)(k - 2 d)
// G = 0 gives the film's mean, G -> (k - 1) / k the median bucket(s).  out = (r, g, b, w).
template <int KP>
SPC_BK_HD void robust_resolve_pixel(const float (*bk)[4], int K, float strength, float* out) {
    float y[KP];
    int rank[KP];
    uint32_t live = 0;
    int k = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < KP; i++) {
        y[i] = 0.0f;
        if (i < K && bk[i][3] > 0.0f) {
            live |= 1u << i;
            k++;
            y[i] = 0.3f * bk[i][0] + 0.6f * bk[i][1] + 0.1f * bk[i][2];
        }
    }
    out[0] = out[1] = out[2] = out[3] = 0.0f;
    if (k == 0) return;
    float T = 0.0f, N = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < KP; i++) {
        int r = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int j = 0; j < KP; j++) {
            const bool before = y[j] < y[i] || (y[j] == y[i] && j < i);
            r += ((live >> j) & 1u) != 0 && before ? 1 : 0;
        }
        rank[i] = r;
        if ((live >> i) & 1u) {
            T += y[i];
            N += (float)(2 * r - k + 1) * y[i];
        }
    }
    float G = 0.0f;
    if (k >= 3 && T > 0.0f) G = fminf(fmaxf(N / ((float)k * T), 0.0f), 1.0f);
    const float t = ((strength * G) * (float)k) * 0.5f;
    const int half = (k - 1) / 2, ft = (int)floorf(t);
    const int d = ft < half ? ft : half;
    float s[3] = {0.0f, 0.0f, 0.0f}, W = 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < KP; i++) {
        if (((live >> i) & 1u) && rank[i] >= d && rank[i] < k - d) {
            const float n = bk[i][3];
            s[0] += n * bk[i][0]; s[1] += n * bk[i][1]; s[2] += n * bk[i][2];
            W += n;
        }
    }
    out[0] = s[0] / W; out[1] = s[1] / W; out[2] = s[2] / W;
    out[3] = (float)(k - 2 * d);
}

}  // namespace spc
