// Per-ray entry point of the POOLED traversal pass (spcbpt_debug_trace_pool; tests/test_gpu_ray_verdict.py).
//
// trace_pool (dev_traversal.h) traces about nine tenths of the eye megakernel's rays and is otherwise seen only through films.  This
// kernel gives one wave exactly what an iteration of k_spcbpt gives it -- per lane an optional own (closest-hit) ray and an eye
// vertex, per (lane, connection) a shadow-ray slot -- runs ONE pass, and writes every answer back ray by ray: each lane's HitRec and
// the slot lengths (trace_pool answers an occluded shadow ray by setting its length to -1).
// The frame is the megakernel's (eye_kernel_body.h): its block size, its TravStack instantiation, its LDS hot-node table filled the
// same way with the same EYE_HOT, pool_ray_list and trace_pool between the same wave-scope fences.  What the eye kernel does around
// the pass (regeneration, connections, shading) is not here.  The constants below are kernels.hip's; tests/test_ray_verdict_cpu.py
// holds the two files to the same text.
#include <hip/hip_runtime.h>

#include "device_lib.h"
#include "kernel_config.h"
#include "kernels.h"

namespace spc {

#ifndef SPC_EYE_BLOCK
#define SPC_EYE_BLOCK 256
#endif
static constexpr int EYE_BLOCK = SPC_EYE_BLOCK;
static constexpr int EYE_HOT = SPC_EYE_BLOCK >= 1024 ? 64 : (SPC_EYE_BLOCK >= 512 ? 38 : 19);   // node records [0, EYE_HOT) live in LDS
static_assert(EYE_HOT <= HOT_NODES, "the builder numbers HOT_NODES nodes first (layout.h)");
#ifndef SPC_EYE_WAVES
#define SPC_EYE_WAVES 4
#endif

struct PoolTraceArgs {
    int n;                     // lanes given by the caller; lane i of the launch is lane i % 64 of wave i / 64
    const float* own_rays;     // n x 8: origin3, -, direction3, -   (the pass's own interval: kEps .. 1e16)
    const int32_t* own_mask;   // n: != 0 = the lane traces its own ray
    const float* shadow_org;   // n x 4: the lane's eye vertex (origin of its shadow rays), -
    float* shadow_rays;        // n x SPCBPT_CONNECTION_N x 4: direction3, length (< 0: empty slot); out: the length of an occluded ray is -1
    float* out_t; int* out_tri; float* out_uv;   // n: the own ray's HitRec (tri in the caller's numbering, -1 = miss or no own ray)
};

__global__ __launch_bounds__(EYE_BLOCK, SPC_EYE_WAVES) void k_debug_trace_pool(const KParams p, const PoolTraceArgs A) {
    constexpr int BLOCK = EYE_BLOCK;
    __shared__ uint32_t s_stack[BLOCK * STACK_LDS];
    struct alignas(16) WavePool {
        float4 ray[POOL_RAYS];      // shadow ray it * 64 + lane: direction.xyz, length (< 0: none)
        float4 org[64];             // eye vertex of lane l
        uint8_t job[POOL_RAYS];     // the slots that hold a ray, compacted (pool_ray_list)
        uint32_t next;              // pool cursor
        uint32_t pad[3];
    };
    __shared__ WavePool s_pool[BLOCK / 64];
    __shared__ float4 s_hot[EYE_HOT * 4];
    const DeviceScene& S = p.scene;
    for (int i = (int)threadIdx.x; i < EYE_HOT * 4; i += BLOCK) s_hot[i] = i < S.tri_base * 4 ? ldq(S.nodes, (size_t)i) : make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave_in_block = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    WavePool* wp = s_pool + wave_in_block;
    uint8_t* w_job = wp->job;
    float4* w_ray = wp->ray;
    float4* w_org = wp->org;
    uint32_t* w_next = &wp->next;
    Counts<false> cn;
    cn.clear();
    TravStack<BLOCK, STACK_LDS> st;
    st.init(s_stack, p.spill, p.spill_entries, (size_t)blockIdx.x * BLOCK + threadIdx.x, p.diag);

    // every lane of the launch runs the pass (trace_pool is a wave-wide call); a lane past the caller's n holds nothing
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool given = i < (long long)A.n;
    bool own = false;
    f3 o = mk3(0.0f), d = mk3(0.0f, 0.0f, 1.0f);
    float4 org = make_float4(0.f, 0.f, 0.f, 0.f);
    if (given) {
        own = A.own_mask[i] != 0;
        if (own) {
            const float4 ra = ldq(A.own_rays, (size_t)i * 2), rb = ldq(A.own_rays, (size_t)i * 2 + 1);
            o = mk3(ra.x, ra.y, ra.z); d = mk3(rb.x, rb.y, rb.z);
        }
        org = ldq(A.shadow_org, (size_t)i);
    }
    w_org[lane] = org;
#pragma unroll
    for (int it = 0; it < SPCBPT_CONNECTION_N; it++)
        w_ray[it * 64 + lane] = given ? ldq(A.shadow_rays, (size_t)i * SPCBPT_CONNECTION_N + it) : make_float4(0.f, 0.f, 0.f, -1.0f);

    // ---- the traversal pass, as eye_kernel_body.h runs it
    if (lane == 0) *w_next = 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint32_t n_rays = pool_ray_list(w_ray, w_job);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    HitRec h;
    trace_pool(S, st, own, o, d, h, w_org, w_ray, w_next, w_job, n_rays, cn, s_hot, EYE_HOT);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();

    if (given) {
        A.out_t[i] = h.t;
        A.out_tri[i] = h.tri >= 0 ? S.tri_orig[h.tri] : -1;
        A.out_uv[2 * i] = h.u; A.out_uv[2 * i + 1] = h.v;
#pragma unroll
        for (int it = 0; it < SPCBPT_CONNECTION_N; it++) A.shadow_rays[((size_t)i * SPCBPT_CONNECTION_N + it) * 4 + 3] = w_ray[it * 64 + lane].w;
    }
}

int trace_pool_debug_threads(int n) { return (n + EYE_BLOCK - 1) / EYE_BLOCK * EYE_BLOCK; }
void launch_trace_pool_debug(const KParams& p, int n, const float* own_rays, const int32_t* own_mask, const float* shadow_org, float* shadow_rays,
                             float* out_t, int* out_tri, float* out_uv, hipStream_t s) {
    PoolTraceArgs A;
    A.n = n; A.own_rays = own_rays; A.own_mask = own_mask; A.shadow_org = shadow_org; A.shadow_rays = shadow_rays;
    A.out_t = out_t; A.out_tri = out_tri; A.out_uv = out_uv;
    hipLaunchKernelGGL(k_debug_trace_pool, dim3(trace_pool_debug_threads(n) / EYE_BLOCK), dim3(EYE_BLOCK), 0, s, p, A);
}

}  // namespace spc
