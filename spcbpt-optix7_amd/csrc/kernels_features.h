// Launcher of the first-hit feature pass (kernels_features.hip).  Declared here and not in kernels.h, which is part of the eye
// megakernel's source hash (source_hash.py: KERNEL_SOURCES).
#pragma once
#include <hip/hip_runtime.h>

#include "layout.h"

namespace spc {

struct FeatureParams;                                            // dev_features.h
int feature_thread_count(const FeatureParams& p);                // threads of the grid (the spill area is sized for it)
void launch_features(const FeatureParams& p, hipStream_t s);     // the launch's rows of p.albedo / p.normal_depth

}  // namespace spc
