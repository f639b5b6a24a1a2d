// spcbpt_local_tone_host: the local tone stage on caller buffers, on the host -- local_tone_pixel.h, the header the kernels of
// kernels_local_tone.hip run, over plain arrays.  No context, no GPU (plain g++, -ffp-contract=off like the device code).  Also the two
// host-only pieces the context shares with it: the parameter check and the plan of the grid.
#include "../../include/spcbpt.h"
#include "local_tone_pixel.h"

#include <vector>

namespace spc {

const char* local_tone_params_error(int cell, float range, int blur, float compress, float detail, float anchor) {
    const float f[4] = {range, compress, detail, anchor};
    for (float v : f)
        if (!isfinite(v)) return "local_tone: a parameter is not a finite number";
    if (cell < 4 || cell > 64) return "local_tone: cell must be 4 .. 64";
    if (!(range >= 0.5f && range <= 8.0f)) return "local_tone: range must be in [0.5, 8]";
    if (blur < 0 || blur > 4) return "local_tone: blur must be 0 .. 4";
    if (!(compress > 0.0f && compress <= 2.0f)) return "local_tone: compress must be in (0, 2]";
    if (!(detail >= 0.0f && detail <= 4.0f)) return "local_tone: detail must be in [0, 4]";
    if (!(anchor > 0.0f)) return "local_tone: anchor must be > 0";
    return nullptr;
}

LtPlan local_tone_plan_of(int width, int height, int cell, float range, float anchor) {
    LtPlan q;
    q.cell = cell;
    q.gx = (width - 1) / cell + 2;
    q.gy = (height - 1) / cell + 2;
    q.nz = (int)(32.0f / range) + 2;
    q.nodes = (int64_t)q.gx * q.gy * q.nz;
    q.la = (float)log2((double)anchor);
    return q;
}

namespace {

struct HostGrid {   // a grid buffer as a plain array of LtNode
    const LtNode* p;
    int gx, nz;
    LtNode operator()(int x, int y, int z) const { return p[((size_t)y * gx + x) * nz + z]; }
};

int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// one blur pass along one axis: `n` nodes along it at `stride`, over every line of the grid
void blur_axis(const std::vector<LtNode>& src, std::vector<LtNode>& dst, const LtPlan& q, int axis) {
    const int dims[3] = {q.gx, q.gy, q.nz};
    const size_t strides[3] = {(size_t)q.nz, (size_t)q.gx * q.nz, 1};
    const int n = dims[axis];
    const size_t st = strides[axis];
    for (int y = 0; y < q.gy; y++)
        for (int x = 0; x < q.gx; x++)
            for (int z = 0; z < q.nz; z++) {
                const int c[3] = {x, y, z};
                const size_t at = ((size_t)y * q.gx + x) * q.nz + z, line = at - (size_t)c[axis] * st;
                dst[at] = lt_blur_node(src[line + (size_t)clampi(c[axis] - 1, n - 1) * st], src[at], src[line + (size_t)clampi(c[axis] + 1, n - 1) * st]);
            }
}

}  // namespace

}  // namespace spc

extern "C" int spcbpt_local_tone_default_params(spcbpt_local_tone_params* p) {
    if (!p) return SPCBPT_ERR_INVALID_ARG;
    p->cell = 16; p->range = 1.0f; p->blur = 1; p->compress = 0.5f; p->detail = 1.0f; p->anchor = 0.18f;
    return SPCBPT_OK;
}

extern "C" int spcbpt_local_tone_params_struct_size(void) { return (int)sizeof(spcbpt_local_tone_params); }

extern "C" int spcbpt_local_tone_host(const float* rgba, int width, int height, const spcbpt_local_tone_params* p, float* out_rgba) {
    using namespace spc;
    if (!rgba || !p || !out_rgba || width < 1 || height < 1 || (int64_t)width * height > (1ll << 28)) return SPCBPT_ERR_INVALID_ARG;
    if (local_tone_params_error(p->cell, p->range, p->blur, p->compress, p->detail, p->anchor)) return SPCBPT_ERR_INVALID_ARG;
    const LtPlan q = local_tone_plan_of(width, height, p->cell, p->range, p->anchor);
    if (q.nodes > kLtMaxNodes) return SPCBPT_ERR_INVALID_ARG;
    const int s = q.cell;
    const size_t px = (size_t)width * height;
    // 1. log-luminance and bin coordinate of the pixels that take part
    std::vector<float> L(px), Z(px);
    std::vector<unsigned char> part(px);
    for (size_t i = 0; i < px; i++) {
        const float Y = lt_luminance(rgba[4 * i], rgba[4 * i + 1], rgba[4 * i + 2]);
        part[i] = lt_takes_part(Y);
        L[i] = part[i] ? lt_loglum(Y) : 0.0f;
        Z[i] = part[i] ? lt_bin(L[i], p->range) : kLtNoBin;
    }
    // 2. the gather: per node the row sums, x ascending, then the rows, ascending
    std::vector<LtNode> grid((size_t)q.nodes), other(p->blur ? (size_t)q.nodes : 0);
    for (int gy = 0; gy < q.gy; gy++)
        for (int gx = 0; gx < q.gx; gx++) {
            const int cx = gx * s, cy = gy * s;
            const int x0 = cx - s + 1 < 0 ? 0 : cx - s + 1, x1 = cx + s - 1 > width - 1 ? width - 1 : cx + s - 1;
            const int y0 = cy - s + 1 < 0 ? 0 : cy - s + 1, y1 = cy + s - 1 > height - 1 ? height - 1 : cy + s - 1;
            for (int gz = 0; gz < q.nz; gz++) {
                LtNode node{0.0f, 0.0f};
                for (int y = y0; y <= y1; y++) {
                    LtNode row{0.0f, 0.0f};
                    for (int x = x0; x <= x1; x++) {
                        const size_t i = (size_t)y * width + x;
                        if (part[i]) lt_row_add(row, lt_tent(x - cx, s), Z[i], L[i], gz);
                    }
                    lt_node_add(node, lt_tent(y - cy, s), row);
                }
                grid[((size_t)gy * q.gx + gx) * q.nz + gz] = node;
            }
        }
    // 3. blur: x over the whole grid, then y, then z, `blur` times
    for (int k = 0; k < p->blur; k++) {
        blur_axis(grid, other, q, 0);
        blur_axis(other, grid, q, 1);
        blur_axis(grid, other, q, 2);
        grid.swap(other);
    }
    // 4, 5. slice and gain
    const HostGrid at{grid.data(), q.gx, q.nz};
    for (int y = 0; y < height; y++)
        for (int x = 0; x < width; x++) {
            const size_t i = (size_t)y * width + x;
            lt_pixel(at, x, y, rgba + 4 * i, s, q.nz, p->range, p->compress, p->detail, q.la, out_rgba + 4 * i);
        }
    return SPCBPT_OK;
}

// test-only: lt_log2 (which 0) or lt_exp2 (which 1) over an array
extern "C" int spcbpt_local_tone_math_host(const float* in, int64_t n, int which, float* out) {
    using namespace spc;
    if (!in || !out || n < 0 || (which != 0 && which != 1)) return SPCBPT_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n; i++) out[i] = which ? lt_exp2(in[i]) : lt_log2(in[i]);
    return SPCBPT_OK;
}
