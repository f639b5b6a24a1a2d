// Stand-alone check of the environment map's sampling table as the product builds it (csrc/env_file.cpp: env_build accumulates in
// float, as upstream's envMapCMFBuild does) against the float64 definition the caller supplies (tests/env_ref.py: table).
//   env_table_check <raster.bin> <reference.bin> <width> <height>
// raster.bin = width x height x 4 float32 as the .hdr stores them (row 0 = top), reference.bin = width x height float64 probabilities.
// A texel's probability is read the way the device reads it (env_pdf: cmf[i] - cmf[i - 1] in float).  Prints one line:
//   size W H zero <texels with probability <= 0> first <env_first_undrawable> first_seen <the first such texel found here>
//   max_rel <largest relative error> median_rel <median> cmf_max_abs <largest |cmf - float64 cmf|> last <cmf[size - 1]>
#include "../../spcbpt-optix7_amd/csrc/env_file.cpp"

#include <algorithm>

int main(int argc, char** argv) {
    if (argc != 5) { fprintf(stderr, "usage: env_table_check raster.bin reference.bin width height\n"); return 2; }
    const int w = atoi(argv[3]), h = atoi(argv[4]);
    if (w < 1 || h < 1 || (long long)w * h > (1ll << 26)) { fprintf(stderr, "bad size\n"); return 2; }
    const size_t size = (size_t)w * h;
    std::vector<float> raster(size * 4);
    std::vector<double> ref(size);
    std::ifstream fr(argv[1], std::ios::binary), fp(argv[2], std::ios::binary);
    fr.read(reinterpret_cast<char*>(raster.data()), (std::streamsize)(raster.size() * sizeof(float)));
    fp.read(reinterpret_cast<char*>(ref.data()), (std::streamsize)(ref.size() * sizeof(double)));
    if (!fr || !fp) { fprintf(stderr, "short input file\n"); return 2; }
    std::vector<float> tex, cmf;
    spc::env_build(raster.data(), w, h, tex, cmf);
    if (tex.size() != size * 4 || cmf.size() != size) { fprintf(stderr, "env_build: wrong table sizes\n"); return 1; }
    for (int j = 0; j < h; j++)          // the texture is the raster with its rows flipped, alpha 1, bit for bit
        for (int i = 0; i < w; i++) {
            const float* q = &raster[((size_t)(h - 1 - j) * w + i) * 4];
            const float* t = &tex[((size_t)j * w + i) * 4];
            if (memcmp(q, t, 12) != 0 || t[3] != 1.0f) { fprintf(stderr, "texture texel (%d, %d) is not raster row %d\n", i, j, h - 1 - j); return 1; }
        }
    std::vector<double> rel(size);
    long long zero = 0, first_seen = -1;
    double max_rel = 0.0, cmf_abs = 0.0, run = 0.0;
    for (size_t i = 0; i < size; i++) {
        const float p = i == 0 ? cmf[0] : cmf[i] - cmf[i - 1];
        if (!(p > 0.0f)) { zero++; if (first_seen < 0) first_seen = (long long)i; }
        rel[i] = fabs((double)p - ref[i]) / ref[i];
        max_rel = std::max(max_rel, rel[i]);
        run += ref[i];
        cmf_abs = std::max(cmf_abs, fabs((double)cmf[i] - run));
    }
    std::nth_element(rel.begin(), rel.begin() + size / 2, rel.end());
    printf("size %d %d zero %lld first %lld first_seen %lld max_rel %.6g median_rel %.6g cmf_max_abs %.6g last %.9g\n", w, h, zero,
           spc::env_first_undrawable(cmf), first_seen, max_rel, rel[size / 2], cmf_abs, (double)cmf[size - 1]);
    // the helper on hand-made tables
    const std::vector<float> ok = {0.25f, 0.5f, 1.0f}, flat = {0.25f, 0.5f, 0.5f, 1.0f}, dark0 = {0.0f, 1.0f}, down = {0.5f, 0.25f, 1.0f};
    if (spc::env_first_undrawable(ok) != -1 || spc::env_first_undrawable(flat) != 2 || spc::env_first_undrawable(dark0) != 0 ||
        spc::env_first_undrawable(down) != 1 || spc::env_first_undrawable(std::vector<float>()) != -1) { fprintf(stderr, "env_first_undrawable: wrong answer on a hand-made table\n"); return 1; }
    return 0;
}
