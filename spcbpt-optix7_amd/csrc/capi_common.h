// Shared prelude of the C ABI's translation units (round 6: capi.hip, 2 000 lines, became seven files):
//   ctx_state.hip     Context: timing spans, buffer sets, the subspace tuple, environment, light-pass geometry, capacities, lifetime
//   ctx_light.hip     Context: light passes (single / batched), the device sampler build (single / batched)
//   ctx_exchange.hip  Context: the shards and imports of a sharded job (what libspcbpt_mgpu drives)
//   ctx_render.hip    Context: eye / pt launches (single, deferred, batched), film merges
//   ctx_features.hip  Context + extern "C": the first-hit feature pass, the a-trous denoiser and the driver the three denoisers share
//   ctx_guides.hip    Context + extern "C": the reflected-guide pass and the switch that makes the two film denoisers read its planes
//   ctx_moments.hip   Context + extern "C": the film's second moment, the film error, the variance-guided denoiser
//   ctx_buckets.hip   Context + extern "C": the bucket film and its median-of-means resolve
//   ctx_display.hip   Context + extern "C": the display transform -- exposure, histogram auto-exposure, tone operators
//                     ... and what the three image-space stages share: their sources, the scratch copy of a caller's image, the plane reader
//   ctx_bloom.hip     Context + extern "C": the bloom stage -- a multi-scale glare ahead of the display transform
//   ctx_local_tone.hip Context + extern "C": the local tone stage -- base / detail through a bilateral grid, ahead of the display transform
//   ctx_history.hip   Context + extern "C": history capture, reprojection into the current view, resolve
//   ctx_lens.hip      Context + extern "C": the thin-lens camera -- its parameters, the host forms of camera_lens.h, the debug ray kernel
//   ctx_adaptive.hip  Context + extern "C": adaptive sampling -- tile counts, tile selection, the list-fed eye launch and its merge
//   capi.hip          extern "C": create / destroy, state, launches by name
//   capi_exchange.hip extern "C": LVC export / import, film band packing
//   capi_debug.hip    extern "C": read-backs, counters, timing, debug and test hooks, preprocessing entry points
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/spcbpt.h"
#include "context.h"
#include "kernels.h"
namespace spc { void launch_repack_nodes_quad2(const float* nodes_q, float* out, int n_nodes, hipStream_t s); }   // quad_trace.hip (declared here: kernels.h is part of the megakernel's source hash)
namespace spc {   // pool_trace.hip (declared here for the same reason)
int trace_pool_debug_threads(int n);
void launch_trace_pool_debug(const KParams& p, int n, const float* own_rays, const int32_t* own_mask, const float* shadow_org, float* shadow_rays,
                             float* out_t, int* out_tri, float* out_uv, hipStream_t s);
}
#include "lbvh.h"
#include "env_host.h"
void spc_viewers_forget_context(spcbpt_ctx* ctx);   // viewer.cpp: called by spcbpt_destroy, so that a viewer outliving its context is safe

#define HIP_TRY(ctx, expr)                                                                       \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess) {                                                                 \
            (ctx)->error = std::string(#expr) + ": " + hipGetErrorString(e__);                   \
            return SPCBPT_ERR_HIP;                                                               \
        }                                                                                        \
    } while (0)

struct spcbpt_ctx : public spc::Context {};

#define CTX_CHECK(c)                                  \
    if (!(c)) return SPCBPT_ERR_INVALID_ARG;          \
    if (hipSetDevice((c)->device) != hipSuccess) { (c)->error = "hipSetDevice failed"; return SPCBPT_ERR_HIP; }
