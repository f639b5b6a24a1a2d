// spcbpt_guide_step_host: the per-bounce arithmetic of the reflected-guide pass on caller arrays, on the host -- guide_step.h, the
// header k_guides runs, over plain arrays.  No context, no GPU (plain g++, -ffp-contract=off like the device code).
#include "../../include/spcbpt.h"
#include "guide_step.h"

extern "C" int spcbpt_guide_step_host(int64_t n, const float* dir, const float* normal, const float* material, const float* specular_tint,
                                      const float* test_normal, const spcbpt_guide_params* params,
                                      int32_t* followed, float* reflected, float* tint, float* unfolded) {
    if (!dir || !normal || !material || !specular_tint || !test_normal || !params || n < 1 || n > (1ll << 28)) return SPCBPT_ERR_INVALID_ARG;
    for (int64_t i = 0; i < n; i++) {
        const float *d = dir + i * 3, *N = normal + i * 3, *m = material + i * 6;
        if (followed) followed[i] = spc::guide_followed(m[4], m[3], params->roughness_max, params->metallic_min) ? 1 : 0;
        if (reflected) spc::guide_reflect(d, N, reflected + i * 3);
        if (tint) spc::guide_tint(m, m[3], m[5], specular_tint[i], N[0] * d[0] + N[1] * d[1] + N[2] * d[2], tint + i * 3);   // dot(N, dir) of device_lib.h
        if (unfolded) spc::guide_reflect(test_normal + i * 3, N, unfolded + i * 3);
    }
    return SPCBPT_OK;
}
