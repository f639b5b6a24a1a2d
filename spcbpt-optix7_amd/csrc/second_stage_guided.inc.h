// The guided second-stage draw of the eye megakernel (eye_kernel_body.h), a TEXT FRAGMENT like eye_kernel_body.h itself:
// included inside a block, once by the megakernel and once by the per-function harness (unit.hip: SPCBPT_UNIT_STAGE2_GUIDED), so that
// what the tests draw through is the product's code and not a restatement of it.  binary_sample (cuProg.h:245-264) of the
// CONNECTION_N connections through the guide table (dev_sampling.h: guide_window).
// In scope at the place of inclusion:
//   const float* f_cmfs, const uint32_t* f_guide   the sampler's CMFs and guide table
//   int bias_[N], size_[N]; float u2_[N]           per connection: the light subspace's record (size 0: skipped) and the random number
//   int lslot_[N]; float pmf2_[N]                  results: the place in the sorted cache (bias + bin) and the bin's probability
//   COUNT, CACHE (compile-time bools), cn (Counts<COUNT>)
                        GuideScan s_[SPCBPT_CONNECTION_N];
                        int pos_[SPCBPT_CONNECTION_N], first_[SPCBPT_CONNECTION_N];
                        bool open_[SPCBPT_CONNECTION_N];
                        uint32_t g_[SPCBPT_CONNECTION_N];
#pragma unroll
                        for (int it = 0; it < SPCBPT_CONNECTION_N; it++)
                            g_[it] = size_[it] > 0 ? f_guide[bias_[it] + min((int)(u2_[it] * (float)size_[it]), size_[it] - 1)] : 0u;
#pragma unroll
                        for (int it = 0; it < SPCBPT_CONNECTION_N; it++) {
                            const int c0 = max((int)g_[it] - 1, 0);
                            s_[it].cnt = c0; s_[it].lo = -INFINITY; s_[it].hi = INFINITY;
                            first_[it] = bias_[it] + c0; pos_[it] = first_[it] & ~3;
                            open_[it] = size_[it] > 0;
                            if (COUNT && CACHE && open_[it]) cn.add(C_CMF);   // (the guide entry; the reference-order form charges the bisection's probes below)
                        }
                        // one connection's windows after the other: the three in flight together hold 24 registers of CMF values and spill
                        // (+18 % against one window at a time: profiles/r05_experiments.md, section 22)
#pragma unroll
                        for (int it = 0; it < SPCBPT_CONNECTION_N; it++) {
                            while (open_[it]) {
                                const float4 a = *reinterpret_cast<const float4*>(f_cmfs + pos_[it]);
                                const float4 b = *reinterpret_cast<const float4*>(f_cmfs + pos_[it] + 4);
                                if (COUNT && CACHE) cn.add(C_CMF, GUIDE_WINDOW);
                                guide_window(a, b, pos_[it], first_[it], bias_[it] + size_[it], u2_[it], s_[it]);
                                pos_[it] += GUIDE_WINDOW;
                                open_[it] = !(s_[it].hi < INFINITY) && pos_[it] < bias_[it] + size_[it];
                            }
                        }
#pragma unroll
                        for (int it = 0; it < SPCBPT_CONNECTION_N; it++) {
                            if (size_[it] != 0) {
                                int k = s_[it].cnt;
                                if (k >= size_[it]) {   // no entry above u (the build ends every CMF with 1: not reached): the bisection's last bin
                                    const float* cmf = f_cmfs + bias_[it];
                                    k = size_[it] - 1;
                                    pmf2_[it] = k == 0 ? cmf[k] : cmf[k] - cmf[k - 1];
                                } else {
                                    pmf2_[it] = k == 0 ? s_[it].hi : s_[it].hi - s_[it].lo;
                                }
                                lslot_[it] = bias_[it] + k;   // its record in the sorted cache (what jump[bias + k] names in the cache's own order)
                                if (COUNT && !CACHE) cn.add(C_CMF, (unsigned)bisection_probes(k, size_[it]));
                            }
                        }
