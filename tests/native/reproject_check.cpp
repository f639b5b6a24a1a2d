// Stand-alone run of the reprojection's host forms (csrc/reproject_host.cpp over csrc/reproject_pixel.h, the header the kernels run)
// for the sanitizers: tests/test_reproject_host.py builds this with -fsanitize=address,undefined and runs it on the CPU.
//   reproject_check <in.bin> <out.bin> <width> <height>
// in.bin  = float32: current camera (eye, U, V, W), history camera, (sigma_n, sigma_x, max_history), then four planes of width x
//           height x 4: normal_depth, history normal_depth, history (rgb, n), accum
// out.bin = float32: the prior, resolve(prior, accum, 3), resolve(NULL, accum, 1) -- three planes, compared by the caller
// Every plane lives in a heap block of exactly its size, so a read or a write one element past a plane is reported.
#include "../../spcbpt-optix7_amd/csrc/reproject_host.cpp"

#include <cstdio>
#include <cstdlib>
#include <memory>

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: reproject_check in.bin out.bin width height\n"); return 2; }
    const int w = atoi(argv[3]), h = atoi(argv[4]);
    if (w < 1 || h < 1 || (long long)w * h > (1ll << 24)) { fprintf(stderr, "bad size\n"); return 2; }
    const size_t plane = (size_t)w * h * 4;
    float head[27];
    std::unique_ptr<float[]> nd(new float[plane]), G(new float[plane]), H(new float[plane]), acc(new float[plane]);
    std::unique_ptr<float[]> prior(new float[plane]), res(new float[plane]), film(new float[plane]);
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    bool ok = fread(head, 4, 27, f) == 27;
    for (float* p : {nd.get(), G.get(), H.get(), acc.get()}) ok = ok && fread(p, 4, plane, f) == plane;
    fclose(f);
    if (!ok) { fprintf(stderr, "short input file\n"); return 2; }
    spcbpt_reproject_params p = {head[24], head[25], head[26]};
    int rc = spcbpt_history_reproject_host(head, head + 3, head + 6, head + 9, nd.get(), head + 12, head + 15, head + 18, head + 21, G.get(), H.get(),
                                           w, h, &p, 0.0f, prior.get());
    if (rc) { fprintf(stderr, "spcbpt_history_reproject_host: %d\n", rc); return 1; }
    rc = spcbpt_history_resolve_host(prior.get(), acc.get(), 3, (int64_t)w * h, res.get());
    if (rc) { fprintf(stderr, "spcbpt_history_resolve_host: %d\n", rc); return 1; }
    rc = spcbpt_history_resolve_host(nullptr, acc.get(), 1, (int64_t)w * h, film.get());
    if (rc) { fprintf(stderr, "spcbpt_history_resolve_host without a prior: %d\n", rc); return 1; }
    // what must be refused is refused without touching a buffer
    if (spcbpt_history_resolve_host(prior.get(), acc.get(), 0, (int64_t)w * h, res.get()) != SPCBPT_ERR_INVALID_ARG ||
        spcbpt_history_resolve_host(prior.get(), nullptr, 1, (int64_t)w * h, res.get()) != SPCBPT_ERR_INVALID_ARG ||
        spcbpt_history_reproject_host(head, head + 3, head + 6, head + 9, nd.get(), head + 12, head + 15, head + 18, head + 21, G.get(), H.get(), w, h,
                                      nullptr, 0.0f, prior.get()) != SPCBPT_ERR_INVALID_ARG) { fprintf(stderr, "a bad argument was accepted\n"); return 1; }
    // a history seen from behind and from far off to the side: g <= 0 and clamped tap coordinates, every tap outside
    float back[12];
    for (int k = 0; k < 12; k++) back[k] = head[12 + k];
    for (int k = 0; k < 3; k++) { back[9 + k] = -back[9 + k]; back[k] += 1e6f * head[15 + k]; }
    std::unique_ptr<float[]> none(new float[plane]);
    rc = spcbpt_history_reproject_host(head, head + 3, head + 6, head + 9, nd.get(), back, back + 3, back + 6, back + 9, G.get(), H.get(), w, h, &p, 0.0f, none.get());
    if (rc) { fprintf(stderr, "spcbpt_history_reproject_host (history behind): %d\n", rc); return 1; }
    for (size_t i = 0; i < plane; i++)
        if (none[i] != 0.0f) { fprintf(stderr, "a history that sees nothing of the view left a prior at %zu\n", i); return 1; }
    f = fopen(argv[2], "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    ok = fwrite(prior.get(), 4, plane, f) == plane && fwrite(res.get(), 4, plane, f) == plane && fwrite(film.get(), 4, plane, f) == plane;
    fclose(f);
    if (!ok) { fprintf(stderr, "short write\n"); return 2; }
    printf("reproject_check %d x %d ok\n", w, h);
    return 0;
}
