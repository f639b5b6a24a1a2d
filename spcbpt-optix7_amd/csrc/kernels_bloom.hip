// The bloom stage: a stencil pyramid.  k_bloom_down builds level k from level k - 1 through an LDS tile (level 0 with the threshold step
// fused in: P is never stored), k_bloom_up mixes a level with the upsampled coarser one in place, k_bloom_tail runs the coarse end of
// the pyramid down and back up inside one workgroup's LDS, k_bloom_composite upsamples U_1 and writes the bloom plane.  Every output
// texel is computed by bloom_pixel.h's functions, the ones spcbpt_bloom_host runs, in their order: where the pyramid is cut between
// the per-level kernels and the tail changes no bit.  One lane per output texel, 16-byte loads and stores, a wave on consecutive x.
#include <hip/hip_runtime.h>

#include "kernels_bloom.h"

namespace spc {

static constexpr int kBloomBlock = 256;
static constexpr int kBloomTileW = 64, kBloomTileH = 4;                             // outputs of a down block: one wave per row
static constexpr int kBloomSrcW = 2 * kBloomTileW + 2, kBloomSrcH = 2 * kBloomTileH + 2;   // the 130 x 10 source texels under them
// The source tile is kept with its even and its odd columns apart: the four taps of output x are even[x], odd[x], even[x + 1],
// odd[x + 1], so that consecutive lanes read consecutive 16-byte slots (a plain row would be read at a 32-byte stride, two lanes per
// slot pair).  72 slots per half: the odd half starts half a bank row (8 slots) off the even one, for the staging writes.
static constexpr int kBloomHalf = 72;

struct BloomLevelAt {   // a level as float4 texels in global memory or LDS, clamped addressing (bloom_pixel.h's `at`)
    const float4* p;
    int w, h;
    __device__ BloomPx operator()(int x, int y) const {
        const float4 v = p[(size_t)bloom_clampi(y, h - 1) * w + bloom_clampi(x, w - 1)];
        return BloomPx{v.x, v.y, v.z};
    }
};

struct BloomTileAt {    // the LDS tile of k_bloom_down: filled with clamped texels, addressed by unclamped coordinates
    const float4* t;
    int ox, oy;         // the unclamped source coordinates of the tile's first texel
    __device__ BloomPx operator()(int x, int y) const {
        const int col = x - ox, row = y - oy;
        const float4 v = t[(row * 2 + (col & 1)) * kBloomHalf + (col >> 1)];
        return BloomPx{v.x, v.y, v.z};
    }
};

__device__ inline float4 bloom_f4(const BloomPx& a) { return make_float4(a.r, a.g, a.b, 0.0f); }

// Level k - 1 -> level k.  A block of four waves makes 64 x 4 outputs: it stages the 130 x 10 source texels under them -- every one is
// wanted by up to four outputs -- in LDS with coalesced 16-byte loads (FIRST: through bloom_pre, so that level 0 is P), then every lane
// takes its sixteen taps from the tile.  Coordinates are clamped while staging, so the tile is complete at the image's edge and for
// levels smaller than a tile.  The grid is one-dimensional (a 1 x 2^28 image has more tile rows than a grid has in y).
template <bool FIRST>
__global__ __launch_bounds__(kBloomBlock) void k_bloom_down(const BloomParams p, const int k) {
    __shared__ float4 tile[kBloomSrcH * 2 * kBloomHalf];
    const int sw = p.w[k - 1], sh = p.h[k - 1], dw = p.w[k], dh = p.h[k];
    const unsigned tiles_x = (unsigned)(dw + kBloomTileW - 1) / kBloomTileW;
    const int x0 = (int)(blockIdx.x % tiles_x) * kBloomTileW, y0 = (int)(blockIdx.x / tiles_x) * kBloomTileH;
    const int ox = 2 * x0 - 1, oy = 2 * y0 - 1;
    const float4* src = FIRST ? reinterpret_cast<const float4*>(p.src) : reinterpret_cast<const float4*>(p.pyr) + p.off[k - 1];
    for (int i = threadIdx.x; i < kBloomSrcW * kBloomSrcH; i += kBloomBlock) {
        const int row = i / kBloomSrcW, col = i - row * kBloomSrcW;
        const int sx = bloom_clampi(ox + col, sw - 1), sy = bloom_clampi(oy + row, sh - 1);
        float4 v = src[(size_t)sy * sw + sx];
        if (FIRST) v = bloom_f4(bloom_pre(v.x, v.y, v.z, p.threshold, p.clamp));
        tile[(row * 2 + (col & 1)) * kBloomHalf + (col >> 1)] = v;
    }
    __syncthreads();
    const int x = x0 + (int)(threadIdx.x & 63), y = y0 + (int)(threadIdx.x >> 6);
    if (x >= dw || y >= dh) return;
    BloomPx d = bloom_down(BloomTileAt{tile, ox, oy}, x, y);
    if (k == p.levels) d = bloom_scale(p.g[k], d);   // the coarsest level is stored as U_L = g_L D_L
    (reinterpret_cast<float4*>(p.pyr) + p.off[k])[(size_t)y * dw + x] = bloom_f4(d);
}

// U_k = g_k D_k + up(U_{k+1}), in place: a texel reads itself and four texels of the coarser level (a quarter of the bytes, shared with
// the neighbours: they come from L2).  One lane per texel in index order.
__global__ __launch_bounds__(kBloomBlock) void k_bloom_up(const BloomParams p, const int k) {
    const int w = p.w[k], h = p.h[k];
    const size_t idx = (size_t)blockIdx.x * kBloomBlock + threadIdx.x;
    if (idx >= (size_t)w * h) return;
    const int y = (int)(idx / (size_t)w), x = (int)(idx - (size_t)y * w);
    float4* lvl = reinterpret_cast<float4*>(p.pyr) + p.off[k];
    const BloomLevelAt coarse{reinterpret_cast<const float4*>(p.pyr) + p.off[k + 1], p.w[k + 1], p.h[k + 1]};
    const float4 d = lvl[idx];
    lvl[idx] = bloom_f4(bloom_mix(p.g[k], BloomPx{d.x, d.y, d.z}, bloom_up(coarse, x, y)));
}

// The coarse end in one launch.  One workgroup reads D_j from the scratch, builds D_{j+1} .. D_L in LDS (level k at the texel offset
// off[k] - off[j+1], the scratch's layout), scales the last, mixes back up in place and leaves U_j in the scratch.  The host picks j so
// that the levels fit (bloom_tail_from).  Every step is one lane per output texel in index order, a barrier between the levels.
__global__ __launch_bounds__(kBloomTailThreads) void k_bloom_tail(const BloomParams p, const int j) {
    __shared__ float4 lds[kBloomTailTexels];
    const int L = p.levels;
    const unsigned long long base = p.off[j + 1];
    float4* dj = reinterpret_cast<float4*>(p.pyr) + p.off[j];
    for (int k = j + 1; k <= L; k++) {
        float4* dst = lds + (p.off[k] - base);
        const BloomLevelAt fine{k == j + 1 ? dj : lds + (p.off[k - 1] - base), p.w[k - 1], p.h[k - 1]};
        const int dw = p.w[k], n = dw * p.h[k];
        for (int i = threadIdx.x; i < n; i += kBloomTailThreads) {
            const int y = i / dw, x = i - y * dw;
            BloomPx d = bloom_down(fine, x, y);
            if (k == L) d = bloom_scale(p.g[L], d);
            dst[i] = bloom_f4(d);
        }
        __syncthreads();
    }
    for (int k = L - 1; k > j; k--) {
        float4* lvl = lds + (p.off[k] - base);
        const BloomLevelAt coarse{lds + (p.off[k + 1] - base), p.w[k + 1], p.h[k + 1]};
        const int w = p.w[k], n = w * p.h[k];
        for (int i = threadIdx.x; i < n; i += kBloomTailThreads) {
            const int y = i / w, x = i - y * w;
            const float4 d = lvl[i];
            lvl[i] = bloom_f4(bloom_mix(p.g[k], BloomPx{d.x, d.y, d.z}, bloom_up(coarse, x, y)));
        }
        __syncthreads();
    }
    const BloomLevelAt coarse{lds, p.w[j + 1], p.h[j + 1]};
    const int w = p.w[j], n = w * p.h[j];
    for (int i = threadIdx.x; i < n; i += kBloomTailThreads) {
        const int y = i / w, x = i - y * w;
        const float4 d = dj[i];
        dj[i] = bloom_f4(bloom_mix(p.g[j], BloomPx{d.x, d.y, d.z}, bloom_up(coarse, x, y)));
    }
}

// out = src + s (up(U_1) - P), alpha copied: P is recomputed from the source texel.  One lane per pixel in index order.
__global__ __launch_bounds__(kBloomBlock) void k_bloom_composite(const BloomParams p) {
    const int w = p.w[0], h = p.h[0];
    const size_t idx = (size_t)blockIdx.x * kBloomBlock + threadIdx.x;
    if (idx >= (size_t)w * h) return;
    const int y = (int)(idx / (size_t)w), x = (int)(idx - (size_t)y * w);
    const BloomLevelAt u1{reinterpret_cast<const float4*>(p.pyr) + p.off[1], p.w[1], p.h[1]};
    const float4 v = reinterpret_cast<const float4*>(p.src)[idx];
    const BloomPx P = bloom_pre(v.x, v.y, v.z, p.threshold, p.clamp);
    const BloomPx B = bloom_up(u1, x, y);
    reinterpret_cast<float4*>(p.out)[idx] = make_float4(bloom_composite(v.x, p.strength, B.r, P.r), bloom_composite(v.y, p.strength, B.g, P.g),
                                                         bloom_composite(v.z, p.strength, B.b, P.b), v.w);
}

static bool bloom_ready(const BloomParams& p) { return p.src && p.out && p.pyr && p.levels >= 1 && p.levels <= kBloomMaxLevels && p.w[0] >= 1 && p.h[0] >= 1; }

int bloom_tail_from(const BloomParams& p, size_t max_input) {
    size_t held = 0;   // the texels of the levels j + 1 .. levels
    int j = 0;
    for (int k = p.levels; k >= 2; k--) {
        held += (size_t)p.w[k] * p.h[k];
        if (held > (size_t)kBloomTailTexels || (size_t)p.w[k - 1] * p.h[k - 1] > max_input) break;
        j = k - 1;
    }
    return j;
}

void launch_bloom_down(const BloomParams& p, int k, hipStream_t s) {
    if (!bloom_ready(p) || k < 1 || k > p.levels) return;
    const size_t tiles = (size_t)((p.w[k] + kBloomTileW - 1) / kBloomTileW) * (size_t)((p.h[k] + kBloomTileH - 1) / kBloomTileH);
    if (k == 1) hipLaunchKernelGGL(k_bloom_down<true>, dim3((unsigned)tiles), dim3(kBloomBlock), 0, s, p, k);
    else hipLaunchKernelGGL(k_bloom_down<false>, dim3((unsigned)tiles), dim3(kBloomBlock), 0, s, p, k);
}

void launch_bloom_up(const BloomParams& p, int k, hipStream_t s) {
    if (!bloom_ready(p) || k < 1 || k >= p.levels) return;
    const size_t n = (size_t)p.w[k] * p.h[k];
    hipLaunchKernelGGL(k_bloom_up, dim3((unsigned)((n + kBloomBlock - 1) / kBloomBlock)), dim3(kBloomBlock), 0, s, p, k);
}

void launch_bloom_tail(const BloomParams& p, int j, hipStream_t s) {
    if (!bloom_ready(p) || j < 1 || j >= p.levels) return;
    if (p.off[p.levels] - p.off[j + 1] + (size_t)p.w[p.levels] * p.h[p.levels] > (size_t)kBloomTailTexels) return;   // does not fit: the caller asked bloom_tail_from
    hipLaunchKernelGGL(k_bloom_tail, dim3(1), dim3(kBloomTailThreads), 0, s, p, j);
}

void launch_bloom_composite(const BloomParams& p, hipStream_t s) {
    if (!bloom_ready(p)) return;
    const size_t n = (size_t)p.w[0] * p.h[0];
    hipLaunchKernelGGL(k_bloom_composite, dim3((unsigned)((n + kBloomBlock - 1) / kBloomBlock)), dim3(kBloomBlock), 0, s, p);
}

}  // namespace spc
