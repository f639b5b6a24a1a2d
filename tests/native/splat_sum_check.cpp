// Stand-alone run of the ordered splat sum's host form (csrc/splat_host.cpp over csrc/splat_pixel.h, the header k_lt_gather runs) for
// the sanitizers: tests/test_splat_sum_host.py builds this with -fsanitize=address,undefined and runs it on the CPU.
//   splat_sum_check <in.bin> <out.bin> <n> <width> <height>
// in.bin  = n x 3 float32 (rgb), then n int32 (pixel index; anything outside [0, width * height) means "no record")
// out.bin = width x height x 3 float32: spcbpt_splat_sum_host's film, compared by the caller
// The program also walks the device's own route on the host -- pad key width * height for "no record", a stable sort of (key, index),
// splat_segment_sum per pixel (one lower-bound search, then the run of equal keys) -- and demands the bits of the host form.
// Every array lives in a heap block of exactly its size, so a read or a write one element past an array is reported.
#include "../../spcbpt-optix7_amd/csrc/splat_host.cpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>

int main(int argc, char** argv) {
    if (argc != 6) { fprintf(stderr, "usage: splat_sum_check in.bin out.bin n width height\n"); return 2; }
    const long long n = atoll(argv[3]);
    const int w = atoi(argv[4]), h = atoi(argv[5]);
    if (n < 0 || n > (1ll << 24) || w < 1 || h < 1 || (long long)w * h > (1ll << 24)) { fprintf(stderr, "bad size\n"); return 2; }
    const size_t pixels = (size_t)w * h;
    std::unique_ptr<float[]> rgb(new float[(size_t)n * 3]), out(new float[pixels * 3]), via_index(new float[pixels * 3]);
    std::unique_ptr<int32_t[]> pixel(new int32_t[(size_t)n]);
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    const bool ok_in = fread(rgb.get(), 4, (size_t)n * 3, f) == (size_t)n * 3 && fread(pixel.get(), 4, (size_t)n, f) == (size_t)n;
    fclose(f);
    if (!ok_in) { fprintf(stderr, "short input file\n"); return 2; }
    int rc = spcbpt_splat_sum_host(n ? rgb.get() : nullptr, n ? pixel.get() : nullptr, n, w, h, out.get());
    if (rc) { fprintf(stderr, "spcbpt_splat_sum_host: %d\n", rc); return 1; }
    // what must be refused is refused without touching a buffer
    if (spcbpt_splat_sum_host(rgb.get(), pixel.get(), n, w, h, nullptr) != SPCBPT_ERR_INVALID_ARG ||
        spcbpt_splat_sum_host(rgb.get(), pixel.get(), -1, w, h, out.get()) != SPCBPT_ERR_INVALID_ARG ||
        spcbpt_splat_sum_host(rgb.get(), pixel.get(), n, 0, h, out.get()) != SPCBPT_ERR_INVALID_ARG ||
        (n > 0 && spcbpt_splat_sum_host(nullptr, pixel.get(), n, w, h, out.get()) != SPCBPT_ERR_INVALID_ARG) ||
        (n > 0 && spcbpt_splat_sum_host(rgb.get(), nullptr, n, w, h, out.get()) != SPCBPT_ERR_INVALID_ARG)) { fprintf(stderr, "a bad argument was accepted\n"); return 1; }
    // the device's route: keys with the pad key, a stable sort of (key, index), one segment sum per pixel over float4-strided records
    std::unique_ptr<uint32_t[]> keys(new uint32_t[(size_t)n]), order(new uint32_t[(size_t)n]), sorted(new uint32_t[(size_t)n]);
    std::unique_ptr<float[]> rec(new float[(size_t)n * 4]);
    for (long long i = 0; i < n; i++) {
        keys[i] = (pixel[i] < 0 || (size_t)pixel[i] >= pixels) ? (uint32_t)pixels : (uint32_t)pixel[i];
        for (int k = 0; k < 3; k++) rec[i * 4 + k] = rgb[i * 3 + k];
        memcpy(&rec[i * 4 + 3], &keys[i], 4);
    }
    std::iota(order.get(), order.get() + n, 0u);
    std::stable_sort(order.get(), order.get() + n, [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    for (long long j = 0; j < n; j++) sorted[j] = keys[order[j]];
    size_t added = 0;
    for (size_t p = 0; p < pixels; p++) added += spc::splat_segment_sum(sorted.get(), order.get(), (uint32_t)n, (uint32_t)p, rec.get(), 4, via_index.get() + p * 3);
    size_t valid = 0;
    for (long long i = 0; i < n; i++) valid += keys[i] < pixels;
    if (added != valid) { fprintf(stderr, "the segments hold %zu records, the input %zu\n", added, valid); return 1; }
    if (memcmp(out.get(), via_index.get(), pixels * 12) != 0) { fprintf(stderr, "the sorted-segment sums are not the bits of the host form\n"); return 1; }
    if (spc::splat_lower_bound(sorted.get(), (uint32_t)n, (uint32_t)pixels + 1u) != (uint32_t)n) { fprintf(stderr, "lower bound past the last key\n"); return 1; }
    f = fopen(argv[2], "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    const bool ok_out = fwrite(out.get(), 4, pixels * 3, f) == pixels * 3;
    fclose(f);
    if (!ok_out) { fprintf(stderr, "short write\n"); return 2; }
    printf("splat_sum_check %lld records on %d x %d ok\n", n, w, h);
    return 0;
}
