// Host side of the mesh lights (layout.h: DLight type 2): the sampling table of one light's triangles.  Plain C++, no device.
#pragma once
#include <cstdint>
#include <vector>

namespace spc {

struct MeshLightTable {
    std::vector<int32_t> tri;      // table order -> index into the triangles handed in (degenerate ones are left out)
    std::vector<float> cmf;        // running area fraction, accumulated in double; the last entry is exactly 1
    std::vector<int32_t> patch;    // 0 .. n_patches - 1, non-decreasing along the table
    std::vector<float> tri_area;   // area of each kept triangle (double arithmetic, rounded once)
    double area = 0.0;             // sum of the kept triangles' areas
    int n_patches = 0;             // patches in use: min(asked for, kept triangles)
};

// Orders the triangles with area > 0 along a Morton curve of their centroids (10 bits per axis inside the light's own box, ties by
// input index) and cuts the run into pieces of about equal area.  `indices` = 3 x n_triangles vertex indices into `vertices`.
void build_mesh_light_table(const float* vertices, const uint32_t* indices, int n_triangles, int n_patches, MeshLightTable& out);

// Guide table of the cutpoint search over `cmf` (dev_sampling.h): entry b = the first place k with cmf[k] > b / buckets.
void build_mesh_light_guide(const std::vector<float>& cmf, int buckets, std::vector<uint32_t>& guide);
int mesh_light_guide_buckets(int n_entries);   // a power of two >= the entries, 16 .. 65536

}  // namespace spc
