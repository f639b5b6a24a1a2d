// The body of the path tracer "pt" (kernels.hip: k_pt<COUNT>, k_pt_lens), included INSIDE each __global__ function like
// eye_kernel_body.h -- no #pragma once.  It reads the kernel's parameter `p` and the compile-time flags COUNT and LENS of the including
// kernel; with LENS = false it is k_pt as it was written in kernels.hip, statement for statement.
    __shared__ uint32_t s_stack[BLOCK * STACK_LDS];
    uint32_t x, y;
    const bool active = lane_pixel(p, x, y);
    Counts<COUNT> cn;
    cn.clear();
    if (active) {
        const DeviceScene& S = p.scene;
        TravStack<BLOCK, STACK_LDS> st;
        st.init(s_stack, p.spill, p.spill_entries, (size_t)blockIdx.x * BLOCK + threadIdx.x, p.diag);
        uint32_t seed;
        f3 origin, dir;
        if (LENS) dir = camera_ray_lens(p, x, y, seed, p.subframe, origin);
        else {
            dir = camera_ray(p, x, y, seed);
            origin = ld3(p.eye);
        }
        f3 throughput = mk3(1.0f), result = mk3(0.0f);
        float prd_pdf = 0.0f;
        int depth = 0;
        bool done = false;
        cn.add(C_PIX); cn.add(C_EYE);
        while (true) {
            HitRec h;
            cn.add(C_CLOSEST);
            f3 current = mk3(0.0f), visA = mk3(0.0f), visB = mk3(0.0f);
            if (!traverse<false, COUNT>(S, st, origin, dir, kEps, 1e16f, h, cn)) {
                done = true;  // __miss__constant_radiance (raygen.cu:687-697): the sky is seen by primary rays only
                if (depth == 0 && S.env.valid) result = throughput * env_color(S.env, dir);
            } else {
                const Geom g = local_geometry(S, h);
                Pbr pbr = load_pbr(S, g.mat);
                if (g.emitter) {  // __closesthit__lightsource
                    const DLight& L = S.lights[pbr.light_id];
                    const LightSampleD ls = area_light_at_hit(S, L, g);
                    if (dot(dir, ls.normal) <= 0) {
                        float mis = 1.0f;
                        if (depth != 0) {
                            const float pdf_hit = prd_pdf * fabsf(dot(dir, ls.normal)) / (h.t * h.t);
                            mis = pdf_hit / (ls.pdf + pdf_hit);
                        }
                        result += throughput * ls.emission * mis;
                    }
                    done = true;
                } else {  // __closesthit__radiance
                    color_tex_sample(S, g, pbr, cn);
                    f3 N = g.N;
                    if (dot(N, dir) > 0.f) N = -N;
                    const f3 in_dir = -dir;
                    const float rr = clampf(max3(pbr.base), SPCBPT_MIN_RR_RATE, 1.0f);
                    const int lid = pick_light(S, seed);
                    const DLight& L = S.lights[lid];
                    if (L.type == 1) {   // next-event estimation of the environment map (hit_program.cu:502-518)
                        const f3 direction = env_sample(S.env, seed);
                        const f3 emission = env_color(S.env, direction);
                        const float lpdf = env_pdf(S.env, direction) / (float)S.n_lights;
                        const f3 V = -normalize(dir);
                        const float L_dot_N = dot(direction, N);
                        if (L_dot_N > 0.0f) {
                            // float3 + float adds the scalar to every component: as written upstream (q18); SPCBPT_ENV_PT_SKY_SHADOW_ALONG_DIR:
                            // the point 2 r along the direction (the oracle's pt_env_nee_fixed)
                            const bool along_dir = (S.env.mode & SPCBPT_ENV_PT_SKY_SHADOW_ALONG_DIR) != 0;
                            visA = g.P; visB = along_dir ? g.P + direction * (S.env.r * 2) : g.P + direction + mk3(S.env.r * 2);
                            const f3 eval = bsdf_eval(pbr, N, V, direction);
                            current = throughput * emission / lpdf * eval * L_dot_N;
                        }
                    } else {
                        const LightSampleD ls = area_light_sample(S, L, seed);
                        const f3 dvec = ls.position - g.P;
                        const float L_dist = sqrtf(dot(dvec, dvec));
                        const f3 Ld = dvec / L_dist;
                        const f3 V = -normalize(dir);
                        const float L_dot_LN = dot(-Ld, ls.normal);
                        const float N_dot_L = dot(N, Ld), N_dot_V = dot(N, V);
                        if (N_dot_L > 0.0f && N_dot_V > 0.0f && L_dot_LN > 0.0f) {
                            visA = g.P; visB = ls.position;
                            const f3 eval = bsdf_eval(pbr, N, V, Ld);
                            const float pdf_hit = bsdf_pdf(pbr, N, V, Ld) * fabsf(L_dot_LN) / (L_dist * L_dist) * rr;
                            const float mis = ls.pdf / (pdf_hit + ls.pdf);
                            current = throughput * ls.emission * 1.0f / ls.pdf * N_dot_L * L_dot_LN / L_dist / L_dist * eval * mis;
                        }
                    }
                    origin = g.P;
                    cn.add(C_VERTEX);
                    if (rnd(seed) > rr) {
                        done = true;
                    } else {
                        dir = bsdf_sample(pbr, N, in_dir, seed);
                        const float pdf = bsdf_pdf(pbr, N, in_dir, dir);
                        if (pdf > 0.0f) {
                            throughput *= bsdf_eval(pbr, N, in_dir, dir) * fabsf(dot(dir, N)) / pdf / rr;
                            prd_pdf = pdf * rr;
                        } else {
                            done = true;
                        }
                    }
                }
            }
            if (sum3(current) > 0.0f) {  // the shadow ray is shot by raygen (raygen.cu:134-143)
                const f3 bias = visB - visA;
                const float len = sqrtf(dot(bias, bias));
                HitRec sh;
                cn.add(C_SHADOW);
                if (!traverse<true, COUNT>(S, st, visA, bias / len, kEps, len - kEps, sh, cn)) result += current;
            }
            if (done || depth > 30) break;
            depth += 1;
        }
        film_write(p, x, y, result);
    }
    cn.flush(p.counters);
