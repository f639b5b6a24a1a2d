// Launcher of the reflected-guide pass (kernels_guides.hip).  Declared here and not in kernels.h, which is part of the eye
// megakernel's source hash (source_hash.py: KERNEL_SOURCES).
#pragma once
#include <hip/hip_runtime.h>

#include "layout.h"

namespace spc {

struct GuideParams;                                          // dev_guides.h
int guide_thread_count(const GuideParams& p);                // threads of the grid (the spill area is sized for it)
void launch_guides(const GuideParams& p, hipStream_t s);     // the launch's rows of p.albedo / p.normal_depth

}  // namespace spc
