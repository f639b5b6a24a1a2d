// Stand-alone run of the variance-carrying host forms of the history reprojection and of the history denoiser (csrc/reproject_host.cpp
// and csrc/denoise_host.cpp over csrc/reproject_pixel.h / csrc/denoise_pixel.h, the headers the kernels run) for the sanitizers:
// tests/test_history_variance_host.py builds this with -fsanitize=address,undefined and runs it on the CPU.
//   history_var_check <in.bin> <out.bin> <width> <height>
// in.bin  = float32: current camera (eye, U, V, W), history camera, (sigma_n, sigma_x, max_history), (sigma_v, sigma_n, sigma_x) of the
//           denoiser, then seven planes of width x height x 4: normal_depth, history normal_depth, history (rgb, n), history variance,
//           accum, m2n, albedo
// out.bin = float32: prior, prior variance, resolve_var(prior, 3) and its variance, resolve_var(NULL, 1) and its variance,
//           history_denoise(the first resolve, 3 iterations) -- seven planes, compared by the caller
// Every plane lives in a heap block of exactly its size, so a read or a write one element past a plane is reported.
#include "../../spcbpt-optix7_amd/csrc/denoise_host.cpp"
#include "../../spcbpt-optix7_amd/csrc/reproject_host.cpp"

#include <cstdio>
#include <cstdlib>
#include <memory>

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: history_var_check in.bin out.bin width height\n"); return 2; }
    const int w = atoi(argv[3]), h = atoi(argv[4]);
    if (w < 1 || h < 1 || (long long)w * h > (1ll << 24)) { fprintf(stderr, "bad size\n"); return 2; }
    const size_t plane = (size_t)w * h * 4;
    const int64_t px = (int64_t)w * h;
    float head[30];
    std::unique_ptr<float[]> nd(new float[plane]), G(new float[plane]), H(new float[plane]), HV(new float[plane]), acc(new float[plane]), m2n(new float[plane]),
        alb(new float[plane]);
    std::unique_ptr<float[]> prior(new float[plane]), pv(new float[plane]), res(new float[plane]), rv(new float[plane]), film(new float[plane]), va(new float[plane]),
        den(new float[plane]);
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    bool ok = fread(head, 4, 30, f) == 30;
    for (float* p : {nd.get(), G.get(), H.get(), HV.get(), acc.get(), m2n.get(), alb.get()}) ok = ok && fread(p, 4, plane, f) == plane;
    fclose(f);
    if (!ok) { fprintf(stderr, "short input file\n"); return 2; }
    spcbpt_reproject_params p = {head[24], head[25], head[26]};
    spcbpt_denoise_params dp = {3, head[27], head[28], head[29]};
    int rc = spcbpt_history_reproject_var_host(head, head + 3, head + 6, head + 9, nd.get(), head + 12, head + 15, head + 18, head + 21, G.get(), H.get(), HV.get(),
                                               w, h, &p, 0.0f, prior.get(), pv.get());
    if (rc) { fprintf(stderr, "spcbpt_history_reproject_var_host: %d\n", rc); return 1; }
    rc = spcbpt_history_resolve_var_host(prior.get(), pv.get(), acc.get(), m2n.get(), 3, px, res.get(), rv.get());
    if (rc) { fprintf(stderr, "spcbpt_history_resolve_var_host: %d\n", rc); return 1; }
    rc = spcbpt_history_resolve_var_host(nullptr, nullptr, acc.get(), m2n.get(), 1, px, film.get(), va.get());
    if (rc) { fprintf(stderr, "spcbpt_history_resolve_var_host without a prior: %d\n", rc); return 1; }
    rc = spcbpt_history_denoise_host(res.get(), rv.get(), alb.get(), nd.get(), head, head + 3, head + 6, head + 9, w, h, &dp, den.get());
    if (rc) { fprintf(stderr, "spcbpt_history_denoise_host: %d\n", rc); return 1; }
    // what must be refused is refused without touching a buffer
    spcbpt_denoise_params none_it = dp, nine_it = dp;
    none_it.iterations = 0;
    nine_it.iterations = 9;
    if (spcbpt_history_resolve_var_host(prior.get(), nullptr, acc.get(), m2n.get(), 1, px, res.get(), rv.get()) != SPCBPT_ERR_INVALID_ARG ||
        spcbpt_history_resolve_var_host(nullptr, pv.get(), acc.get(), m2n.get(), 1, px, res.get(), rv.get()) != SPCBPT_ERR_INVALID_ARG ||
        spcbpt_history_resolve_var_host(prior.get(), pv.get(), acc.get(), m2n.get(), 0, px, res.get(), rv.get()) != SPCBPT_ERR_INVALID_ARG ||
        spcbpt_history_resolve_var_host(prior.get(), pv.get(), acc.get(), nullptr, 1, px, res.get(), rv.get()) != SPCBPT_ERR_INVALID_ARG ||
        spcbpt_history_denoise_host(res.get(), rv.get(), alb.get(), nd.get(), head, head + 3, head + 6, head + 9, w, h, &none_it, den.get()) != SPCBPT_ERR_INVALID_ARG ||
        spcbpt_history_denoise_host(res.get(), rv.get(), alb.get(), nd.get(), head, head + 3, head + 6, head + 9, w, h, &nine_it, den.get()) != SPCBPT_ERR_INVALID_ARG ||
        spcbpt_history_denoise_host(res.get(), nullptr, alb.get(), nd.get(), head, head + 3, head + 6, head + 9, w, h, &dp, den.get()) != SPCBPT_ERR_INVALID_ARG ||
        spcbpt_history_reproject_var_host(head, head + 3, head + 6, head + 9, nd.get(), head + 12, head + 15, head + 18, head + 21, G.get(), H.get(), nullptr, w, h,
                                          &p, 0.0f, prior.get(), pv.get()) != SPCBPT_ERR_INVALID_ARG) { fprintf(stderr, "a bad argument was accepted\n"); return 1; }
    // a history seen from behind and from far off to the side: g <= 0 and clamped tap coordinates, every tap outside
    float back[12];
    for (int k = 0; k < 12; k++) back[k] = head[12 + k];
    for (int k = 0; k < 3; k++) { back[9 + k] = -back[9 + k]; back[k] += 1e6f * head[15 + k]; }
    std::unique_ptr<float[]> none(new float[plane]), none_var(new float[plane]);
    rc = spcbpt_history_reproject_var_host(head, head + 3, head + 6, head + 9, nd.get(), back, back + 3, back + 6, back + 9, G.get(), H.get(), HV.get(), w, h, &p, 0.0f,
                                           none.get(), none_var.get());
    if (rc) { fprintf(stderr, "spcbpt_history_reproject_var_host (history behind): %d\n", rc); return 1; }
    for (size_t i = 0; i < plane; i++)
        if (none[i] != 0.0f || none_var[i] != 0.0f) { fprintf(stderr, "a history that sees nothing of the view left a prior or a variance at %zu\n", i); return 1; }
    f = fopen(argv[2], "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    ok = true;
    for (const float* q : {prior.get(), pv.get(), res.get(), rv.get(), film.get(), va.get(), den.get()}) ok = ok && fwrite(q, 4, plane, f) == plane;
    fclose(f);
    if (!ok) { fprintf(stderr, "short write\n"); return 2; }
    printf("history_var_check %d x %d ok\n", w, h);
    return 0;
}
