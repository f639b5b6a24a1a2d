// Host-side set-up of the environment map (env_file.cpp)
#pragma once
#include <vector>

namespace spc {
void env_build(const float* raster, int w, int h, std::vector<float>& tex, std::vector<float>& cmf);
// The first texel the float table can never draw: the first i with cmf[i] <= cmf[i - 1] (or cmf[0] <= 0), else -1.  Every texel's
// probability is at least 0.25 / size by definition, so such an entry is the float accumulation's doing: the map is too large for it.
long long env_first_undrawable(const std::vector<float>& cmf);
}
