// The job list of the eye kernel's connect phase, ordered by kind (eye_kernel_body.h; restated nowhere: tests/native/job_order_check.cpp
// instantiates this header on the host with a wave replayed lane by lane).
//
// A wave holds N x 64 (connection, lane) slots.  After the traversal pass some are alive (an unoccluded pair), and each carries one
// bit of kind: 1 = the light vertex is expected to sit on an emitter (connect_vertices: b.depth == 0, the short arm), 0 = a surface
// vertex (the general arm: a dependent material fetch, two bsdf_eval, three bsdf_pdf).  The list holds the general jobs first, then the
// emitter jobs, each group in (connection, lane) order, so that a round of 64 consecutive jobs is of one kind wherever the counts
// allow it and the wave skips the other arm.  The bit is a scheduling hint: connect_vertices branches on the vertex's own depth, so a
// wrong bit costs time and changes no value, and the owners still add their results in connection order.
//
// 2 N ballots; every lane returns the same count; entry n .. of `job` is not written.  `wave.ballot(b)` is the only collective.
#pragma once
#include <cstdint>

#ifndef SPC_DEV
#define SPC_DEV inline
#define SPC_JOB_ORDER_OWN_DEV_
#endif

namespace spc {

static constexpr uint32_t kJobKindBit = 0x80000000u;   // bit 31 of a WavePool::slot word (a place in the sorted cache is below 2^31)

template <int N, class Wave>
SPC_DEV uint32_t job_list_by_kind(Wave& wave, uint32_t lane, uint32_t my_live, uint32_t my_emitter, uint8_t* job) {
    static_assert(N * 64 <= 256, "a slot number is one byte");
    uint32_t n = 0u;
#pragma unroll
    for (int kind = 0; kind < 2; kind++) {
#pragma unroll
        for (int it = 0; it < N; it++) {
            const bool take = ((my_live >> it) & 1u) != 0u && ((my_emitter >> it) & 1u) == (uint32_t)kind;
            const unsigned long long m = wave.ballot(take);
            if (take) job[n + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = (uint8_t)(it * 64 + lane);
            n += (uint32_t)__builtin_popcountll(m);
        }
    }
    return n;
}

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
struct HwWave {
    __device__ __forceinline__ unsigned long long ballot(bool b) const { return __ballot(b); }
};
#endif

}  // namespace spc

#ifdef SPC_JOB_ORDER_OWN_DEV_
#undef SPC_DEV
#undef SPC_JOB_ORDER_OWN_DEV_
#endif
