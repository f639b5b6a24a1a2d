// The local tone stage: a bilateral grid.  k_lt_build gathers the footprint of one node column into its NZ nodes through LDS,
// k_lt_blur is one blur pass, its three axes in one launch, k_lt_slice interpolates the base layer under every pixel and applies the
// gain.  Every output is computed by local_tone_pixel.h's functions, the ones spcbpt_local_tone_host runs, in their order: how the work
// is cut over lanes, chunks and launches changes no bit.  No atomics: every node and every pixel has one writer.
#include <hip/hip_runtime.h>

#include "kernels_local_tone.h"

namespace spc {

static constexpr int kLtBlock = 256;
static constexpr int kLtTent = 127;      // 2 s - 1 at s = 64: the tent over the offsets -(s - 1) .. s - 1
static constexpr int kLtPix = 2048;      // the most (z, L) pairs of one chunk of footprint rows: 16 KB
static constexpr int kLtSums = 2048;     // the most (a_j, b_j) row sums of one chunk, [row][active bin]: 16 KB
static constexpr int kLtBins = 128;      // the bin tables: two ballots of wave 0 cover them
static_assert(kLtMaxNZ <= kLtBins && kLtBins == 2 * 64 && kLtBins <= kLtBlock, "a lane per bin keeps a node's sums in registers across the chunks");
static_assert(kLtPix >= kLtTent && kLtSums >= kLtMaxNZ, "a chunk holds at least one footprint row");

struct LtGridAt {   // a grid buffer in global memory (local_tone_pixel.h's `at`)
    const float2* p;
    int gx, nz;
    __device__ LtNode operator()(int x, int y, int z) const {
        const float2 v = p[((size_t)y * gx + x) * nz + z];
        return LtNode{v.x, v.y};
    }
};

// One workgroup per node column (gx, gy).  Its footprint, the pixels with |x - gx s| < s and |y - gy s| < s inside the image, is walked
// in chunks of whole rows:
//   (1) the chunk's pixels are staged in LDS as (z, L), computed from the source on the way in -- a pixel that takes no part as
//       (kLtNoBin, 0), whose terms are +-0 -- and every pixel that takes part marks the two bins its tent can reach, floor(z) and
//       floor(z) + 1 (|z - gz| >= 1 for every other bin, and the rounding of the difference cannot bring it below 1);
//   (2) wave 0 turns the marks into the ascending list of the chunk's ACTIVE bins with two ballots;
//   (3) a lane per (row, active bin) walks its row x ascending with broadcast LDS reads and leaves the row sums (a_j, b_j) in LDS;
//   (4) the lane that owns a bin adds the chunk's rows, ascending, to the node it keeps in registers.
// A bin that is not active has a_j = b_j = +0 in every row of the chunk, and adding wy 0 to a node changes no bit (a sum that starts
// at +0 never becomes -0), so leaving those bins out is the definition's sum.  An image whose neighbourhoods span a few stops has a
// few active bins of NZ; with every bin marked, the list and its barrier cost 4 %.
// Step (4) of a chunk reads what the staging of the next one does not write, so a chunk costs three barriers.
// The two large arrays are sized per launch (lt_build_lds): the blocks a CU holds, not the arithmetic, bound this kernel.
__global__ __launch_bounds__(kLtBlock) void k_lt_build(const LocalToneParams p, const int dst, const int n_pix, const int n_sums) {
    extern __shared__ float2 lt_lds[];
    __shared__ float tent[kLtTent + 1];
    __shared__ int mark[kLtBins], active[kLtBins], slot[kLtBins], n_active;
    float2* pix = lt_lds;             // n_pix (z, L) pairs
    float2* sums = lt_lds + n_pix;    // n_sums row sums
    const int tid = (int)threadIdx.x, s = p.cell, nz = p.nz;
    const int gy = (int)(blockIdx.x / (unsigned)p.gx), gx = (int)(blockIdx.x - (unsigned)gy * (unsigned)p.gx);
    const int cx = gx * s, cy = gy * s;
    const int x0 = cx - s + 1 < 0 ? 0 : cx - s + 1, x1 = cx + s - 1 > p.width - 1 ? p.width - 1 : cx + s - 1;
    const int y0 = cy - s + 1 < 0 ? 0 : cy - s + 1, y1 = cy + s - 1 > p.height - 1 ? p.height - 1 : cy + s - 1;
    const int fw = x1 - x0 + 1;
    float2* out = reinterpret_cast<float2*>(p.grid[dst]) + (size_t)blockIdx.x * nz;
    LtNode node{0.0f, 0.0f};
    if (fw >= 1 && y1 >= y0) {   // (the last column and row of nodes may have no pixel at all)
        for (int i = tid; i < 2 * s - 1; i += kLtBlock) tent[i] = lt_tent(i - (s - 1), s);
        if (tid < kLtBins) mark[tid] = 0;
        __syncthreads();
        const int by_pix = n_pix / fw, by_sums = n_sums / nz;
        const int rows = by_pix < by_sums ? by_pix : by_sums;
        const float4* src = reinterpret_cast<const float4*>(p.src);
        for (int yc = y0; yc <= y1; yc += rows) {
            const int rc = y1 - yc + 1 < rows ? y1 - yc + 1 : rows;
            for (int i = tid; i < rc * fw; i += kLtBlock) {
                const int row = i / fw, col = i - row * fw;
                const float4 v = src[(size_t)(yc + row) * p.width + (x0 + col)];
                const float Y = lt_luminance(v.x, v.y, v.z);
                float2 zl = make_float2(kLtNoBin, 0.0f);
                if (lt_takes_part(Y)) {
                    zl.y = lt_loglum(Y);
                    zl.x = lt_bin(zl.y, p.range);
                    int iz = (int)zl.x;                      // 0 <= z <= 32 / range, so 0 <= floor(z) and floor(z) + 1 <= NZ - 1 as it is
                    iz = iz < 0 ? 0 : (iz > nz - 2 ? nz - 2 : iz);
                    mark[iz] = 1;                                            // (every writer writes the same 1)
                    mark[iz + 1] = 1;
                }
                pix[i] = zl;
            }
            __syncthreads();
            if (tid < 64) {   // wave 0: bin tid and bin 64 + tid
                const int m0 = mark[tid], m1 = mark[64 + tid];
                const unsigned long long b0 = __ballot(m0 != 0), b1 = __ballot(m1 != 0), below = (1ull << tid) - 1ull;
                const int n0 = __popcll(b0), r0 = __popcll(b0 & below), r1 = n0 + __popcll(b1 & below);
                slot[tid] = m0 ? r0 : -1;
                slot[64 + tid] = m1 ? r1 : -1;
                if (m0) active[r0] = tid;
                if (m1) active[r1] = 64 + tid;
                if (tid == 0) n_active = n0 + __popcll(b1);
                mark[tid] = 0;                               // for the next chunk
                mark[64 + tid] = 0;
            }
            __syncthreads();
            const int na = n_active;
            for (int k = tid; k < rc * na; k += kLtBlock) {
                const int row = k / na, gz = active[k - row * na];
                const float2* line = pix + row * fw;
                const float* wx = tent + (x0 - cx + s - 1);
                LtNode sum{0.0f, 0.0f};
                for (int col = 0; col < fw; col++) {
                    const float2 zl = line[col];
                    lt_row_add(sum, wx[col], zl.x, zl.y, gz);
                }
                sums[k] = make_float2(sum.a, sum.b);
            }
            __syncthreads();
            if (tid < nz && slot[tid] >= 0) {
                const float* wy = tent + (yc - cy + s - 1);
                const float2* mine = sums + slot[tid];
                for (int row = 0; row < rc; row++) {
                    const float2 r = mine[row * na];
                    lt_node_add(node, wy[row], LtNode{r.x, r.y});
                }
            }
        }
    }
    if (tid < nz) out[tid] = make_float2(node.a, node.b);
}

// One blur pass: along x, then y, then z, in one launch.  A lane per node: the x pass at the nine (y, z) neighbours it needs, clamped,
// the y pass at the three z neighbours, the z pass -- each value by the arithmetic the pass over the whole grid would use, so the bits
// are those of three passes.  27 reads per node, neighbours in z adjacent in memory and the others NZ and GX NZ nodes apart, shared
// with the neighbouring lanes (L1 / L2); a third of the launches and of the traffic of three one-axis passes.
__global__ __launch_bounds__(kLtBlock) void k_lt_blur(const LocalToneParams p, const int from) {
    const size_t n = (size_t)p.gx * p.gy * p.nz;
    const size_t idx = (size_t)blockIdx.x * kLtBlock + threadIdx.x;
    if (idx >= n) return;
    const size_t cell = idx / (size_t)p.nz;
    const int z = (int)(idx - cell * (size_t)p.nz), y = (int)(cell / (size_t)p.gx), x = (int)(cell - (size_t)y * p.gx);
    const int xs[3] = {x > 0 ? x - 1 : 0, x, x < p.gx - 1 ? x + 1 : x}, ys[3] = {y > 0 ? y - 1 : 0, y, y < p.gy - 1 ? y + 1 : y};
    const int zs[3] = {z > 0 ? z - 1 : 0, z, z < p.nz - 1 ? z + 1 : z};
    const LtGridAt at{reinterpret_cast<const float2*>(p.grid[from]), p.gx, p.nz};
    LtNode along_y[3];
    for (int k = 0; k < 3; k++) {
        LtNode along_x[3];
        for (int j = 0; j < 3; j++) along_x[j] = lt_blur_node(at(xs[0], ys[j], zs[k]), at(xs[1], ys[j], zs[k]), at(xs[2], ys[j], zs[k]));
        along_y[k] = lt_blur_node(along_x[0], along_x[1], along_x[2]);
    }
    const LtNode o = lt_blur_node(along_y[0], along_y[1], along_y[2]);
    reinterpret_cast<float2*>(p.grid[1 - from])[idx] = make_float2(o.a, o.b);
}

// Slice and gain: one lane per pixel in index order, a 16-byte load and a 16-byte store.  The eight nodes under a pixel are read from
// the grid in global memory: neighbouring lanes read the same nodes and the grid is a few megabytes at most, so they come from L1 / L2
// (staging the node columns under a 64 x 4 tile in LDS first measured 40 % slower: DESIGN.md 8l).
__global__ __launch_bounds__(kLtBlock) void k_lt_slice(const LocalToneParams p, const int from) {
    const size_t idx = (size_t)blockIdx.x * kLtBlock + threadIdx.x;
    if (idx >= (size_t)p.width * p.height) return;
    const int y = (int)(idx / (size_t)p.width), x = (int)(idx - (size_t)y * p.width);
    const LtGridAt at{reinterpret_cast<const float2*>(p.grid[from]), p.gx, p.nz};
    const float4 v = reinterpret_cast<const float4*>(p.src)[idx];
    const float in[4] = {v.x, v.y, v.z, v.w};
    float o[4];
    lt_pixel(at, x, y, in, p.cell, p.nz, p.range, p.compress, p.detail, p.la, o);
    reinterpret_cast<float4*>(p.out)[idx] = make_float4(o[0], o[1], o[2], o[3]);
}

static bool local_tone_ready(const LocalToneParams& p) {
    return p.src && p.out && p.grid[0] && p.grid[1] && p.width >= 1 && p.height >= 1 && p.cell >= 4 && p.cell <= 64 && p.nz >= 2 && p.nz <= kLtMaxNZ &&
           p.gx == (p.width - 1) / p.cell + 2 && p.gy == (p.height - 1) / p.cell + 2 && (int64_t)p.gx * p.gy * p.nz <= kLtMaxNodes;
}

void launch_local_tone_build(const LocalToneParams& p, int dst, hipStream_t s) {
    if (!local_tone_ready(p) || (dst != 0 && dst != 1)) return;
    // a whole footprint and its row sums where they fit, else chunks of rows: at least one row of 2 s - 1 pixels and of NZ sums either way
    const int side = 2 * p.cell - 1;
    const int n_pix = side * side < kLtPix ? side * side : kLtPix, n_sums = side * p.nz < kLtSums ? side * p.nz : kLtSums;
    hipLaunchKernelGGL(k_lt_build, dim3((unsigned)((size_t)p.gx * p.gy)), dim3(kLtBlock), (size_t)(n_pix + n_sums) * sizeof(float2), s, p, dst, n_pix, n_sums);
}

void launch_local_tone_blur(const LocalToneParams& p, int src, hipStream_t s) {
    if (!local_tone_ready(p) || (src != 0 && src != 1)) return;
    const size_t n = (size_t)p.gx * p.gy * p.nz;
    hipLaunchKernelGGL(k_lt_blur, dim3((unsigned)((n + kLtBlock - 1) / kLtBlock)), dim3(kLtBlock), 0, s, p, src);
}

void launch_local_tone_slice(const LocalToneParams& p, int src, hipStream_t s) {
    if (!local_tone_ready(p) || (src != 0 && src != 1)) return;
    const size_t n = (size_t)p.width * p.height;
    hipLaunchKernelGGL(k_lt_slice, dim3((unsigned)((n + kLtBlock - 1) / kLtBlock)), dim3(kLtBlock), 0, s, p, src);
}

}  // namespace spc
