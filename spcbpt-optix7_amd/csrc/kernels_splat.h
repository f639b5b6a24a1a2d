// Launchers of the light-tracing estimator "lt" (kernels_splat.hip).  Declared here and not in kernels.h, which is part of the eye
// megakernel's source hash (source_hash.py: KERNEL_SOURCES).
#pragma once
#include <hip/hip_runtime.h>

#include "layout.h"

namespace spc {

struct SplatParams;                                                   // dev_splat.h
int splat_blocks(int max_blocks);                                     // persistent grid of k_lt_splat (the spill area is sized for it)
int splat_block_threads();
void launch_lt_splat(const SplatParams& p, int blocks, hipStream_t s);   // p.splat must have been zeroed on `s`
void launch_lt_resolve(const SplatParams& p, hipStream_t s);             // splat -> p.result over the launch's rows
// the ordered mode (spcbpt_set_splat_order): records -> [a stable sort of (p.keys, p.vals) over p.bound items] -> gather
void launch_lt_records(const SplatParams& p, int blocks, hipStream_t s); // every slot of p.records / keys / vals in [0, p.bound) written once
void launch_lt_gather(const SplatParams& p, hipStream_t s);              // p.keys_sorted / vals_sorted / records -> p.result over the launch's rows

}  // namespace spc
