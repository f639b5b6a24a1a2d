// Launchers of the display transform (kernels_display.hip): luminance histogram, auto exposure, tone map.  Declared here and not in
// kernels.h, which is part of the eye megakernel's source hash (source_hash.py: KERNEL_SOURCES).
#pragma once
#include <hip/hip_runtime.h>

#include "display_pixel.h"

namespace spc {

// The pass's device record, one allocation of kDisplayStateWords uint32: the 258 counters of the histogram, then the adaptation
// state -- the bits of the last auto EV (float) and whether there is one.
static constexpr int kDisplayStateEv = kDisplayCounters, kDisplayStateHavePrev = kDisplayCounters + 1, kDisplayStateWords = kDisplayCounters + 2;

struct DisplayParams {  // passed by value as the kernel argument block of the three kernels
    size_t pixels;
    const float* src;       // float4 per pixel, index order (read only)
    uint32_t* frame;        // RGBA8 out
    uint32_t* state;        // kDisplayStateWords words (see above)
    int op;                 // 0 FILM, 1 REINHARD, 2 ACES, 3 LINEAR
    int auto_ev;            // 1: k_display_map takes EV from state[kDisplayStateEv], 0: from `ev`
    float ev, white;
    DisplayExposure exposure;
};
void launch_display_histogram(const DisplayParams& p, hipStream_t s);   // src -> state[0 .. 257] (ADDS: the caller zeroes them first)
void launch_display_exposure(const DisplayParams& p, hipStream_t s);    // counters, previous EV -> EV, have_prev = 1
void launch_display_map(const DisplayParams& p, hipStream_t s);         // src, EV -> frame

}  // namespace spc
