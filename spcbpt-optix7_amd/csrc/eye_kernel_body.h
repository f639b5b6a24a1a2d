// The body of the eye megakernel (kernels.hip: k_spcbpt, k_spcbpt_sky), included INSIDE each __global__ function -- no #pragma once.
// It reads the kernel's parameter `p` and the compile-time flags COUNT, BATCH, CACHE, ENV, SKY, TILES and LENS of the including kernel.  (As the
// body of one force-inlined device function called by both kernels the timed forms came out with other code: the kernel argument
// is then reached through a generic pointer, and the early passes schedule around it differently.  Included, k_spcbpt<...> is
// compiled from the same statements as before SKY existed: tests/test_codegen_guard.py, tools/codegen_diff_symbols.py.)
    constexpr int BLOCK = EYE_BLOCK;   // (this kernel's; the other kernels of the file run 256-thread blocks)
    __shared__ uint32_t s_stack[BLOCK * STACK_LDS];
    // everything else a wave keeps in LDS sits in ONE record per wave: every field is then the wave's base (one SGPR) plus a
    // constant that folds into the ds instruction's offset.  As eight separate arrays the eight wave-uniform bases were spilled
    // SGPRs, read back with v_readlane inside the traversal loop.
    struct alignas(16) WavePool {
        float4 ray[POOL_RAYS];      // shadow ray it * 64 + lane: direction.xyz, length (< 0: none)
        float4 org[64];             // eye vertex of lane l: position.xyz (= origin of its shadow rays), lastNormalProjection
        int32_t slot[POOL_RAYS];    // LVC slot of connection it * 64 + lane; bit 31: its kind (job_order.h: kJobKindBit)
        float pmf[POOL_RAYS];       // its resampling pmf (path_count * pmf2 * pmf1)
        uint8_t job[POOL_RAYS];     // before the pass: slots that hold a ray; after it: the unoccluded connections, compacted
                                    // (the pass answers a shadow ray in the ray's own slot: an occluded pair's length becomes -1 = no ray)
        uint32_t next;              // pool cursor
        uint32_t pad[3];
    };
    __shared__ WavePool s_pool[BLOCK / 64];
    // the hottest nodes of the BVH (layout.h: HOT_NODES, numbered first by the builder), one copy per block
    __shared__ float4 s_hot[EYE_HOT * 4];
    const DeviceScene& S = p.scene;
    for (int i = (int)threadIdx.x; i < EYE_HOT * 4; i += BLOCK) s_hot[i] = i < S.tri_base * 4 ? ldq(S.nodes, (size_t)i) : make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    // wave_in_block through readfirstlane: the per-wave LDS base below is then a wave-uniform value the compiler keeps in an SGPR
    const uint32_t lane = threadIdx.x & 63, wave_in_block = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    WavePool* wp = s_pool + wave_in_block;
    int32_t* w_slot = wp->slot;
    float* w_pmf = wp->pmf;
    uint8_t* w_job = wp->job;
    uint32_t* w_stack = s_stack + wave_in_block * 64;      // [entry * BLOCK + lane]: free between two traversal passes
    float4* w_ray = wp->ray;
    float4* w_org = wp->org;
    uint32_t* w_next = &wp->next;
    Counts<COUNT> cn;
    cn.clear();
    TravStack<BLOCK, STACK_LDS> st;
    st.init(s_stack, p.spill, p.spill_entries, (size_t)blockIdx.x * BLOCK + threadIdx.x, p.diag);
    const int path_count = BATCH ? 0 : p.sampler_counts[1];
    const uint32_t n_tiles = BATCH ? p.n_tiles * p.n_frames : p.n_tiles;   // queue length
    uint32_t fid = 0, pool_fid = 0, pend_fid = 0;   // frame of the lane's path / of the wave's current tile / of the parked pixel

    bool alive = false, exhausted = false;
    uint32_t pool_tile = 0;
    uint32_t pool_sample = 0;   // TILES: the sample index of the wave's current tile (wave-uniform; what p.subframe is to the other forms)
    int pool_left = 0;
    uint32_t xy = 0;   // the pixel of the lane's path, x | y << 16: one register across the pass (the packing of `pend_xy`)
    WalkState w;
    EyeVertex cur;
    f3 result = mk3(0.0f);
    w.done = false; w.seed = 0; w.origin = w.dir = w.next_flux = mk3(0.0f); w.next_single_pdf = 1.0f;
    cur.c.pos = cur.c.n = cur.c.color = cur.c.lastPos = mk3(0.0f); cur.c.lnp = 0.0f; cur.c.mat = 0; cur.c.lld = false;
    cur.flux = cur.R3 = mk3(0.0f); cur.pdf = cur.singlePdf = 1.0f; cur.sub = cur.lastZone = cur.depth = 0; cur.lsub = 0;

    // software pipeline: the vertex built in iteration i is connected in iteration i + 1, in the same traversal pass that
    // extends the path by its next segment (the next direction is drawn before the connections, hit_program.cu:324-337)
    bool has_vertex = false, has_ray = false;
    // A path that ended at a vertex (Russian roulette / depth) still owes that vertex's connections, which are evaluated one
    // iteration later.  Its lane does not wait for them: it parks the pixel and the radiance so far (`pend_*`), starts the next
    // pixel-sample at once (`fresh`: the camera vertex is installed after the connect phase, which still reads `cur`), and
    // writes the parked pixel when the connections have been added.
    // Where the parked radiance waits: the kernel spills, and what is alive across the traversal pass is what it spills.  A single-frame
    // launch accumulates through film_write and keeps `pend_result` in registers.  A BATCH launch stores each frame's samples with a plain
    // store to that frame's own film, which nothing else touches before k_film_merge_batch (a pixel-sample of a frame belongs to one lane;
    // the batched form refuses while film moments are on): there the lane stores `result` when it parks, and only an owner one of whose
    // owed connections came back unoccluded reads the value again after the connect phase, adds its contributions in connection order and
    // stores the sum.  The value returns from memory bit for bit, so the chain of FP32 additions is the single-frame form's.
    // (Measured, profiles/r08_experiments.md: 144 -> 128 B of scratch per lane in the batched plain form, 160 -> 128 B in the general one;
    // the read issued BEFORE the job loop, to cover its latency, keeps six more registers alive through connect_vertices and spills more.)
    bool pend_valid = false, fresh = false;
    uint32_t pend_xy = 0;
    f3 pend_result = mk3(0.0f);
#pragma unroll
    for (int it = 0; it < SPCBPT_CONNECTION_N; it++) w_ray[it * 64 + lane] = make_float4(0.f, 0.f, 0.f, -1.0f);
    const unsigned long long w_start = COUNT ? wall_clock64() : 0ull;
    long long t_ph = COUNT ? clock64() : 0;
#define SPC_PHASE(slot) do { if (COUNT) { const long long t1__ = clock64(); if (lane == 0) cn.add(slot, (unsigned)((t1__ - t_ph) >> 4)); t_ph = t1__; } } while (0)
    while (true) {
        // ---- regeneration: hand pixel-samples of the pool to idle lanes
        unsigned long long idle = __ballot(!alive || !has_ray);
        while (idle != 0ull && !exhausted) {
            if (pool_left == 0) {
                uint32_t t = 0;
                if (lane == (uint32_t)__ffsll((long long)idle) - 1u) t = atomicAdd(p.work_counter, 1u);
                t = __shfl(t, __ffsll((long long)idle) - 1, 64);
                if (t >= n_tiles) { exhausted = true; break; }
                if (TILES) {   // the queue is a list of tiles of the whole film, each at a sample index of its own (t < n_tiles = the list's length)
                    pool_tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.tile_list[t]);
                    pool_sample = (uint32_t)__builtin_amdgcn_readfirstlane((int)p.tile_samples[pool_tile]);
                }
                else pool_tile = BATCH ? t % p.n_tiles : t;
                pool_fid = BATCH ? t / p.n_tiles : 0u;
                pool_left = 64;
            }
            const int n_idle = __popcll(idle);
            const int take = n_idle < pool_left ? n_idle : pool_left;
            const int my_rank = __popcll(idle & ((1ull << lane) - 1ull));
            if ((!alive || !has_ray) && my_rank < take) {
                const uint32_t slot = (uint32_t)(64 - pool_left + my_rank);
                uint32_t nx, ny;
                if (tile_pixel(p, pool_tile, slot, nx, ny)) {
                    if (alive) {
                        pend_valid = true; pend_xy = xy; pend_fid = fid;
                        if (BATCH) film_store(p.frames[fid].result, p.width, xy & 0xffffu, xy >> 16, result);   // parked in the frame's film
                        else pend_result = result;
                    }
                    xy = nx | (ny << 16);
                    fid = pool_fid;
                    alive = true;
                    has_ray = true;
                    fresh = true;
                    if (LENS) w.dir = camera_ray_lens(p, nx, ny, w.seed, p.subframe, w.origin);   // (dev_lens.h: the lens point, and the ray through the sample's focus point)
                    else {
                        w.dir = camera_ray(p, nx, ny, w.seed, TILES ? pool_sample : (BATCH ? p.frames[fid].subframe : p.subframe));
                        w.origin = ld3(p.eye);
                    }
                    w.done = false;
                    w.next_flux = mk3(0.0f);
                    w.next_single_pdf = 1.0f;
                    result = mk3(0.0f);
                    cn.add(C_PIX); cn.add(C_EYE);
                }
            }
            pool_left -= take;
            // slots that fall outside the image (partial tiles) are consumed; their lanes stay idle for this round
            const unsigned long long still = __ballot(!alive || !has_ray);
            if (still == idle && pool_left > 0) break;  // only out-of-image slots were handed out: avoid spinning
            idle = still;
        }
        if (!__any(alive)) {
            if (exhausted) break;
            continue;
        }
        SPC_PHASE(C_T_REGEN);
        // ---- traversal pass: the next segment of every live path and the shadow rays of the vertices built last iteration
        if (lane == 0) *w_next = 0u;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // the slots that hold a shadow ray, compacted (w_job is free here: the connect phase below rebuilds it after the pass)
        const uint32_t n_rays = pool_ray_list(w_ray, w_job);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // the vertex's five small integers cross the pass in two registers (the pass needs every register it can get: the kernel spills)
        const uint32_t ids_a = (uint32_t)cur.sub | ((uint32_t)cur.lastZone << 10) | ((uint32_t)cur.depth << 20);
        const uint32_t ids_b = (uint32_t)cur.c.mat | ((uint32_t)cur.lsub << 16);
        HitRec h;
        // (the next segment starts at the path's last vertex -- or at the camera for a path that was started in this iteration, whose
        // `cur` still holds the parked path's vertex: w.origin would be a copy kept alive across the pass for nothing.  LENS: the camera is
        // the lane's own lens point, which only w.origin holds -- that form keeps the three registers from the regeneration to init_EyeSubpath)
        // Issue priority by phase (s_setprio): the traversal pass is the phase whose instructions are the kernel's throughput (three quarters
        // of what it issues), connect and shading are chains of dependent fetches with little to issue in between -- a wave in the pass
        // goes first when both are ready.  Measured (profiles/r05_experiments.md, section 16): pass 1 / others 0: +1.1 % paths per second;
        // any phase but the pass raised: the light pass that shares the CUs (priority 0 throughout) starves and the step gets longer.
        if (SPC_PRIO_TRAV != SPC_PRIO_SHADE) __builtin_amdgcn_s_setprio(SPC_PRIO_TRAV);
        trace_pool(S, st, alive && has_ray, fresh ? (LENS ? w.origin : ld3(p.eye)) : cur.c.pos, w.dir, h, w_org, w_ray, w_next, w_job, n_rays, cn, s_hot, EYE_HOT);
        if (SPC_PRIO_CONNECT != SPC_PRIO_TRAV) __builtin_amdgcn_s_setprio(SPC_PRIO_CONNECT);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        cur.sub = (int)(ids_a & 1023u); cur.lastZone = (int)((ids_a >> 10) & 1023u); cur.depth = (int)(ids_a >> 20);
        cur.c.mat = (int)(ids_b & 0xffffu); cur.lsub = (int)(ids_b >> 16);
        SPC_PHASE(C_T_POOL);
        // ---- connect the unoccluded pairs of the previous vertices.  Most of the 192 (lane, connection) slots of a wave hold none
        // (on the bench workload a pass leaves ~158 jobs in ~3.2 rounds: profiles/r10_experiments.md), so the pairs are compacted
        // into a job list and every lane -- whatever the state of its
        // own path -- evaluates one job per round: the eye vertices are published through the (now idle) traversal-stack
        // LDS, the results come back through the ray slots and each owner adds its own in connection order, which keeps
        // the floating-point sums identical to evaluating them in place.
        // The list is ordered by kind (job_order.h): connections to surface light vertices first, to emitter vertices after them,
        // so that whole rounds run one arm of connect_vertices only.  The kind is the bit the draw left in the slot word.
        {
            uint32_t my_live = 0u, my_emitter = 0u;
#pragma unroll
            for (int it = 0; it < SPCBPT_CONNECTION_N; it++) {
                const bool live = has_vertex && w_ray[it * 64 + lane].w >= 0.0f;   // a ray was shot and found nothing in the way
                // (selects, no branch: with `if (live)` around the two the kernel's scratch grows from 128 to 144 B per lane)
                my_live |= (uint32_t)live << it;
                my_emitter |= (uint32_t)(live && w_slot[it * 64 + lane] < 0) << it;
            }
            HwWave hw;
            const uint32_t n_jobs = job_list_by_kind<SPCBPT_CONNECTION_N>(hw, lane, my_live, my_emitter, w_job);
            if (n_jobs != 0u) {
                if (my_live) {  // publish this lane's eye vertex (position and lastNormalProjection already sit in w_org)
                    uint32_t* col = w_stack + lane;
                    col[0 * BLOCK] = __float_as_uint(cur.c.n.x); col[1 * BLOCK] = __float_as_uint(cur.c.n.y); col[2 * BLOCK] = __float_as_uint(cur.c.n.z);
                    col[3 * BLOCK] = __float_as_uint(cur.c.color.x); col[4 * BLOCK] = __float_as_uint(cur.c.color.y); col[5 * BLOCK] = __float_as_uint(cur.c.color.z);
                    col[6 * BLOCK] = __float_as_uint(cur.c.lastPos.x); col[7 * BLOCK] = __float_as_uint(cur.c.lastPos.y); col[8 * BLOCK] = __float_as_uint(cur.c.lastPos.z);
                    col[9 * BLOCK] = __float_as_uint(cur.flux.x); col[10 * BLOCK] = __float_as_uint(cur.flux.y); col[11 * BLOCK] = __float_as_uint(cur.flux.z);
                    col[12 * BLOCK] = __float_as_uint(cur.pdf); col[13 * BLOCK] = __float_as_uint(cur.singlePdf);
                    // the frame of the VERTEX: a lane that parked its pixel has already taken a tile of possibly another frame
                    col[14 * BLOCK] = (uint32_t)cur.sub | ((uint32_t)cur.lastZone << 10) | ((uint32_t)cur.depth << 20) | ((pend_valid ? pend_fid : fid) << 26);   // depth <= 51 (raygen.cu:361): 6 bits; frame id: 6 bits
                    col[15 * BLOCK] = (uint32_t)cur.c.mat | ((uint32_t)cur.lsub << 16);   // material ids are < 32768 (spcbpt_create)
                    // (RMIS_pointer_3 does not fit the 16 stack entries four resident blocks leave: it travels by ds_bpermute below)
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                for (uint32_t base = 0; base < n_jobs; base += 64u) {   // wave-uniform: the shuffles below need every lane
                    const uint32_t j = base + lane;
                    const bool job = j < n_jobs;
                    const uint32_t slot = job ? w_job[j] : 0u, owner = slot & 63u;
                    const f3 ownerR3 = mk3(__shfl(cur.R3.x, (int)owner, 64), __shfl(cur.R3.y, (int)owner, 64), __shfl(cur.R3.z, (int)owner, 64));
                    if (COUNT) { if (job) cn.add(C_U_JOB_LANES); if (lane == 0) cn.add(C_U_JOB_SLOTS, 64); }
                    if (!job) continue;
                    const uint32_t* col = w_stack + owner;
                    const float4 po = w_org[owner];
                    EyeVertex a;
                    a.c.pos = mk3(po.x, po.y, po.z); a.c.lnp = po.w; a.c.lld = false;
                    a.c.n = mk3(__uint_as_float(col[0 * BLOCK]), __uint_as_float(col[1 * BLOCK]), __uint_as_float(col[2 * BLOCK]));
                    a.c.color = mk3(__uint_as_float(col[3 * BLOCK]), __uint_as_float(col[4 * BLOCK]), __uint_as_float(col[5 * BLOCK]));
                    a.c.lastPos = mk3(__uint_as_float(col[6 * BLOCK]), __uint_as_float(col[7 * BLOCK]), __uint_as_float(col[8 * BLOCK]));
                    a.flux = mk3(__uint_as_float(col[9 * BLOCK]), __uint_as_float(col[10 * BLOCK]), __uint_as_float(col[11 * BLOCK]));
                    a.R3 = ownerR3;
                    a.pdf = __uint_as_float(col[12 * BLOCK]); a.singlePdf = __uint_as_float(col[13 * BLOCK]);
                    const uint32_t ids = col[14 * BLOCK];
                    a.sub = (int)(ids & 1023u); a.lastZone = (int)((ids >> 10) & 1023u); a.depth = (int)((ids >> 20) & 63u);
                    const LightVertex* job_lvc = BATCH ? p.frames[ids >> 26].lvc_sorted : p.lvc_sorted;   // (w_slot holds the vertex's place in the sampler's order)
                    a.c.mat = (int)(col[15 * BLOCK] & 0xffffu); a.lsub = (int)(col[15 * BLOCK] >> 16);
                    LightVertex b;
                    const float4* src = reinterpret_cast<const float4*>(job_lvc + ((uint32_t)w_slot[slot] & ~kJobKindBit));
                    const float job_pmf = w_pmf[slot];
                    float4* dst = reinterpret_cast<float4*>(&b);
#pragma unroll
                    for (int q = 0; q < 6; q++) dst[q] = src[q];
                    f3 res = connect_vertices<COUNT, CACHE, ENV>(p, a, b, cn);
                    if (is_invalid(res)) res = mk3(0.0f);
                    res = res / job_pmf;
                    const bool ok = !is_invalid(res);
                    res = res / (float)SPCBPT_CONNECTION_N;
                    w_ray[slot] = make_float4(res.x, res.y, res.z, ok ? 1.0f : 0.0f);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                // BATCH: a parked pixel that is owed a connection comes back from its frame's film
                float4* pend_px = nullptr;
                f3 sum = result;
                if (pend_valid) {
                    if (!BATCH) sum = pend_result;
                    else if (my_live) {
                        pend_px = reinterpret_cast<float4*>(p.frames[pend_fid].result) + ((size_t)(pend_xy >> 16) * p.width + (pend_xy & 0xffffu));
                        const float4 parked = *pend_px;
                        sum = mk3(parked.x, parked.y, parked.z);
                    }
                }
#pragma unroll
                for (int it = 0; it < SPCBPT_CONNECTION_N; it++) {
                    if (my_live & (1u << it)) {
                        const float4 r = w_ray[it * 64 + lane];
                        if (r.w != 0.0f) sum += mk3(r.x, r.y, r.z);
                    }
                }
                if (!pend_valid) result = sum;
                else if (!BATCH) pend_result = sum;
                else if (my_live) *pend_px = make_float4(sum.x, sum.y, sum.z, 1.0f);   // (film_store's record)
            }
        }
        if (pend_valid) {
            if (!BATCH) film_write(p, pend_xy & 0xffffu, pend_xy >> 16, pend_result);   // (BATCH: the pixel already stands in its frame's film)
            pend_valid = false;
        }
        if (fresh) {  // init_EyeSubpath (raygen.cu:216-231)
            fresh = false;
            cur.c.pos = LENS ? w.origin : ld3(p.eye); cur.c.n = w.dir; cur.c.color = mk3(0.0f); cur.c.lastPos = cur.c.pos; cur.c.lnp = 0.0f; cur.c.mat = 0; cur.c.lld = false;
            cur.flux = mk3(1.0f); cur.R3 = mk3(0.0f); cur.pdf = 1.0f; cur.singlePdf = 1.0f; cur.sub = 0; cur.lastZone = 0; cur.depth = 0; cur.lsub = 0;
        }
        has_vertex = false;
        bool finished = alive && !has_ray;  // the path ended at that vertex (Russian roulette / depth): nothing was traced
        SPC_PHASE(C_T_CONNECT);
        if (SPC_PRIO_SHADE != SPC_PRIO_CONNECT) __builtin_amdgcn_s_setprio(SPC_PRIO_SHADE);
        // ---- the new segment: miss, emitter, or a new vertex with its CONNECTION_N resampled light vertices
        if (alive && has_ray) {
            has_ray = false;
            if (h.tri < 0) {
                finished = true;  // __miss__BDPTVertex
                if (SKY) result += eye_sky_miss<COUNT, CACHE, ENV>(p, w.dir, cur.depth == 0, cur, w, cn);   // (the same accumulator as an emitter hit)
            } else {
                const Geom g = local_geometry(S, h);
                const bool last_is_origin = cur.depth == 0;
                const f3 ray_dir = w.dir;
                if (g.emitter) {
                    result += eye_emitter_hit<COUNT, CACHE, ENV>(p, g, h.t, ray_dir, last_is_origin, cur, w, cn);
                    finished = true;
                } else {
                    EyeVertex mid;
                    eye_surface_hit<COUNT, CACHE, ENV>(p, g, h.t, ray_dir, last_is_origin, cur, w, mid, cn, true);
                    cur = mid;
                    has_vertex = true;
                    long long t_s0 = COUNT ? clock64() : 0;
                    // CONNECTION_N resampled connections through the subspace sampling matrix (raygen.cu:390-419).  Only the
                    // position quad of the light vertex is fetched here (visibilityTest, cuProg.h:463-487); the connection
                    // itself does not consume random numbers, so drawing all three first leaves the RNG stream unchanged.
                    // (the light vertices in the sampler's order: the vertex drawn at place k of a subspace's CMF is record jump_bias + k,
                    // next to the other vertices of its subspace -- no trip through `jump`)
                    const LightVertex* f_lvc = p.lvc_sorted; const DSubspace* f_subspace = p.subspace; const float* f_cmfs = p.cmfs; const uint32_t* f_guide = p.guide;
                    int f_path_count = path_count;
                    const int32_t* f_counts = p.sampler_counts;
                    if (BATCH) {   // the sampler tables of this path's frame
                        const FrameDesc& D = p.frames[fid];
                        f_lvc = D.lvc_sorted; f_subspace = D.subspace; f_cmfs = D.cmfs; f_guide = D.guide; f_path_count = D.sampler_counts[1];
                        f_counts = D.sampler_counts;
                    }
                    // Three stages, each over all CONNECTION_N connections:
                    // (1) per connection, in order (the random numbers are one stream, and an empty subspace draws none for its second stage):
                    //     the light subspace and its record; (2) sampleSecondStage of each through the guide table, one window at a time;
                    //     (3) the sampled slots, the light vertices' position quads and the rays.
                    // (The first stages side by side on a guessed stream, and the second-stage windows in flight together, save round trips and
                    // LOSE: they cost registers in a kernel that spills -- profiles/r05_experiments.md, sections 4 and 22.)
                    float pmf1_[SPCBPT_CONNECTION_N], pmf2_[SPCBPT_CONNECTION_N], u2_[SPCBPT_CONNECTION_N];
                    int lslot_[SPCBPT_CONNECTION_N], bias_[SPCBPT_CONNECTION_N], size_[SPCBPT_CONNECTION_N];
#pragma unroll
                    for (int it = 0; it < SPCBPT_CONNECTION_N; it++) { pmf1_[it] = 1.0f; pmf2_[it] = 0.0f; u2_[it] = 0.0f; lslot_[it] = -1; bias_[it] = 0; size_[it] = 0; }
#pragma unroll
                    for (int it = 0; it < SPCBPT_CONNECTION_N; it++) {
                        // The connection's kind, the connect phase's scheduling hint (job_order.h): the drawn light subspace is an emitter patch's
                        // (the light tree's labels end below them), so the vertex drawn from it sits on an emitter; 0 for the comparator.  It waits
                        // in the slot word itself -- a register kept through the second stage is a register spilled -- and stage (3) ORs the place in.
                        if (p.uniform_lvc) {   // the comparator of BASELINE config 5: uniformSample (cuProg.h:283-289), one random number
                            w_slot[it * 64 + lane] = 0;
                            const int vc = f_counts[0];
                            if (vc > 0) lslot_[it] = uniform_sample_index(vc, w.seed, pmf2_[it]);   // (place in the jump buffer = record of the sorted cache)
                        } else {
                            const int l = sample_first_stage<COUNT, CACHE>(p, cur.sub, w.seed, pmf1_[it], cn);
                            w_slot[it * 64 + lane] = l >= SPCBPT_NUM_SUBSPACE - SPCBPT_NUM_SUBSPACE_LIGHTSOURCE ? (int32_t)kJobKindBit : 0;
                            const DSubspace ss = f_subspace[l];
                            if (ss.size != 0) { bias_[it] = ss.jump_bias; size_[it] = ss.size; u2_[it] = rnd(w.seed); }
                        }
                    }
                    {   // binary_sample (cuProg.h:245-264) of the three through the guide table (device_lib.h: guide_window); every sampler build
                        // writes one (capi.hip: set_guide is allocated with the CMF), so there is no bisection beside it
#include "second_stage_guided.inc.h"
                    }
#pragma unroll
                    for (int it = 0; it < SPCBPT_CONNECTION_N; it++) {
                        const float pmf1 = pmf1_[it], pmf2 = pmf2_[it];
                        const int lslot = lslot_[it];
                        float4 rq = make_float4(0.f, 0.f, 0.f, -1.0f);
                        if (lslot >= 0) {
                            __hip_atomic_fetch_or(&w_slot[it * 64 + lane], lslot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);   // (one ds_or_b32: the lane's own word, under its kind bit)
                            cn.add(C_CONN);
                            const float4 bq0 = reinterpret_cast<const float4*>(f_lvc + lslot)[0];
                            const float4 bq1 = reinterpret_cast<const float4*>(f_lvc + lslot)[1];
                            w_pmf[it * 64 + lane] = (float)f_path_count * pmf2 * pmf1;
                            // a light vertex that is a DIRECTION of the environment map (only scenes with one pay the flag fetch):
                            // visibilityTest shoots from the eye vertex to eye - 10 r n_b (cuProg.h:489-495)
                            const bool b_dir = ENV && (f_lvc[lslot].pad & SPCBPT_LV_DIRECTION) != 0u;
                            const f3 target = b_dir ? -10 * S.env.r * mk3(bq1.x, bq1.y, bq1.z) + cur.c.pos : mk3(bq0.x, bq0.y, bq0.z);
                            const f3 bias = target - cur.c.pos;
                            const float len = sqrtf(dot(bias, bias));
                            const f3 sdir = bias / len;
                            // a pair that faces away on either side has a BSDF factor of exactly zero (bsdf_eval / the one-sided
                            // emitter term of connect_vertices): its shadow ray cannot change the pixel and is not traced
                            if (b_dir ? !null_connection_direction(cur.c.n, mk3(bq1.x, bq1.y, bq1.z))
                                      : !null_connection(cur.c.pos, cur.c.n, mk3(bq0.x, bq0.y, bq0.z), mk3(bq1.x, bq1.y, bq1.z)))
                                rq = make_float4(sdir.x, sdir.y, sdir.z, len);
                        }
                        w_ray[it * 64 + lane] = rq;
                    }
                    if (COUNT) cn.add(C_T_SAMPLE, (unsigned)((clock64() - t_s0) >> 4));
                    w_org[lane] = make_float4(cur.c.pos.x, cur.c.pos.y, cur.c.pos.z, cur.c.lnp);
                    // the loop-top test of raygen.cu:361: a path that ends here still connects this vertex (next iteration)
                    has_ray = !(w.done || cur.depth > 50);   // (cur.depth = the number of segments traced: raygen.cu:361 counts them in payload.depth)
                }
            }
        }
        if (!has_vertex) {
#pragma unroll
            for (int it = 0; it < SPCBPT_CONNECTION_N; it++) w_ray[it * 64 + lane] = make_float4(0.f, 0.f, 0.f, -1.0f);
        }
        if (alive && finished) {
            if (BATCH) film_store(p.frames[fid].result, p.width, xy & 0xffffu, xy >> 16, result);
            else film_write(p, xy & 0xffffu, xy >> 16, result);
            alive = false;
        }
        SPC_PHASE(C_T_SHADE);
    }
#undef SPC_PHASE
    if (COUNT && p.counters && lane == 0) {
        const unsigned long long w_end = wall_clock64();
        atomicMin(&p.counters[C_W_START_MIN], w_start);
        atomicMax(&p.counters[C_W_END_MAX], w_end);
        atomicAdd(&p.counters[C_W_END_SUM], w_end);
        atomicAdd(&p.counters[C_W_WAVES], 1ull);
    }
    cn.flush(p.counters);
