"""The bloom stage on the host -- the per-texel code the kernels run (csrc/bloom_pixel.h) behind spcbpt_bloom_host -- against the float64
numpy definition of tests/bloom_ref.py, on synthetic images.  Needs no GPU.

The bar, per finite channel:   |O - O_ref| <= (32 L + 16) 2^-24 (|I_c| + s (B0_c + C_c)) + 1e-30
with C the clipped source and B0 its blur (the same run with threshold 0).  Derived, u = 2^-24:
  * every term of the pyramid is non-negative, so rounding errors stay relative to the exact value: a down level is a horizontal and a
    vertical sum of four products, 7 roundings each on the longest path plus the two weights' products, at most ~20 u; an up-and-mix
    level is two lerps (3 roundings each), the product with g_k and its one rounding to float, and the sum: at most ~8 u; L levels of
    both stay under 32 L u of B <= B0;
  * the threshold step's t = (Y - T) / Y has an absolute error of at most ~8 u (Y carries 5 roundings, the difference and the quotient
    one each, relative to Y), so P is off by at most ~8 u C, which a non-negative operator of unit gain turns into at most 8 u B0;
  * the composite adds 3 roundings on |I| + s (B + P).
16 u cover the last two.  The +1e-30 covers channels whose products fall below the normal range.
That the bar separates a right result from a wrong one is checked here too: three mutants of the reference (zero padding instead of the
edge clamp, 0.25 / 0.75 swapped in `up`, the coarsest level dropped) miss it on every shape larger than 1 x 1."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import bloom_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
IDS = [f"{w}x{h}" for w, h in ref.SIZES]
GRID = [(L, q, T) for L in ref.LEVELS for q in ref.SPREADS for T in ref.THRESHOLDS]
STRENGTH = 0.7


@pytest.fixture(scope="module")
def images():
    return {f"{w}x{h}": ref.planted_image(w, h) for w, h in ref.SIZES}


# ------------------------------------------------------------------------------------------------------------ against the definition
@pytest.mark.parametrize("name", IDS)
def test_host_form_meets_the_bar(pkg, images, name):
    img, plants = images[name]
    worst = 0.0
    for L, q, T in GRID:
        kw = dict(levels=L, strength=STRENGTH, spread=q, threshold=T)
        out = pkg.api.bloom_host(img, **kw)
        r = ref.bloom(img, **kw)
        assert out.dtype == np.float32 and out.shape == img.shape
        assert np.array_equal(out[..., 3], img[..., 3])                                  # alpha is the source's
        assert np.array_equal(np.isnan(out), np.isnan(img)), (name, kw)                   # a NaN stays in its channel, and only there
        assert np.array_equal(np.isinf(out), np.isinf(img)) and (out[np.isinf(img)] > 0).all()
        ratio, n = ref.excess(out, img, r, L, STRENGTH)
        worst = max(worst, ratio)
        assert n == img[..., :3].size - len(plants["nan"]) - len(plants["inf"])
        assert ratio <= 1.0, (name, kw, ratio)
        for (y, x, c) in plants["inf"]:                                                   # the neighbours of +inf are finite (and judged above)
            y0, y1, x0, x1 = max(y - 2, 0), min(y + 3, img.shape[0]), max(x - 2, 0), min(x + 3, img.shape[1])
            assert np.isfinite(out[y0:y1, x0:x1, :3][np.isfinite(img[y0:y1, x0:x1, :3])]).all()
    print(f"{name}: worst |O - O_ref| / bar over the grid {worst:.3f}")


@pytest.mark.parametrize("name", IDS[1:])
@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_bar_rejects_the_mutants(images, name, mutant):
    """The reference itself, made wrong in one place, against the right reference: outside the bar at every shape and L."""
    img, _ = images[name]
    for L in ref.LEVELS:
        kw = dict(levels=L, strength=STRENGTH)
        r = ref.bloom(img, **kw)
        wrong = ref.bloom(img, mutant=mutant, **kw)["O"]
        ratio, _ = ref.excess(wrong, img, r, L, STRENGTH)
        assert ratio > 1.0, (name, mutant, L, ratio)
    assert ref.excess(ref.bloom(img, levels=3, strength=STRENGTH)["O"], img, ref.bloom(img, levels=3, strength=STRENGTH), 3, STRENGTH)[0] == 0.0


# ------------------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("name", IDS)
def test_constant_image_comes_back(pkg, name):
    w, h = (int(v) for v in name.split("x"))
    img = np.full((h, w, 4), 0.5, np.float32)
    for L in ref.LEVELS:
        assert np.array_equal(pkg.api.bloom_host(img, levels=L), img), (name, L)
        assert np.abs(ref.bloom(img, levels=L, strength=1.0)["O"] - 0.5).max() < 1e-15


@pytest.mark.parametrize("name", IDS)
def test_strength_zero_and_high_threshold_return_the_source(pkg, name):
    w, h = (int(v) for v in name.split("x"))
    img = ref.seeded_image(w, h)
    top = float(ref.bloom(img)["C"].max())                 # above every luminance: the weights sum to 1
    for L in ref.LEVELS:
        assert np.array_equal(pkg.api.bloom_host(img, levels=L, strength=0.0, spread=2.0), img)
        assert np.array_equal(pkg.api.bloom_host(img, levels=L, strength=1.0, threshold=top + 1.0), img)


@pytest.mark.parametrize("L", [1, 2, 3])
def test_light_is_neither_created_nor_lost(pkg, L):
    """Two impulses at the centre of a 64 x 96 image.  The condition first: the REFERENCE's B is zero on the outermost rows and columns,
    so nothing reached the border, where the clamp would fold light back.  Then the sums agree within the sum of the per-texel bars."""
    img = ref.impulse_image(64, 96)
    kw = dict(levels=L, strength=0.5, spread=1.5)
    r = ref.bloom(img, **kw)
    B = r["B"]
    assert B.max() > 0 and not B[0].any() and not B[-1].any() and not B[:, 0].any() and not B[:, -1].any()
    assert abs(r["O"][..., :3].sum() / img[..., :3].astype(np.float64).sum() - 1.0) < 1e-14
    out = pkg.api.bloom_host(img, **kw).astype(np.float64)
    bars = ref.bound(img, r, L, 0.5)
    for c in range(3):
        assert abs(out[..., c].sum() - img[..., c].astype(np.float64).sum()) <= bars[..., c].sum(), (L, c)
    assert (out[..., :3] > 0).sum() > (img[..., :3] > 0).sum()          # and it did spread


def test_result_does_not_depend_on_the_neighbours_of_a_nan(pkg):
    """A NaN gives nothing to the pyramid: replacing it by zero changes its own channel only."""
    img, plants = ref.planted_image(43, 29)
    clean = img.copy()
    for (y, x, c) in plants["nan"]:
        clean[y, x, c] = 0.0
    a, b = pkg.api.bloom_host(img, levels=3, strength=0.5), pkg.api.bloom_host(clean, levels=3, strength=0.5)
    differ = a.view(np.uint32) != b.view(np.uint32)
    assert sorted(map(tuple, np.argwhere(differ))) == sorted(plants["nan"])


# ------------------------------------------------------------------------------------------------------------ the ABI
def test_defaults_struct_size_and_abi_count(pkg, hip_lib):
    p = pkg.api.bloom_params()
    assert (p.levels, p.strength, p.spread, p.threshold, p.clamp) == (5, np.float32(0.1), 1.0, 0.0, 65504.0)
    assert hip_lib.spcbpt_bloom_params_struct_size() == C.sizeof(pkg.api.BloomParams) == 20
    sizes = (C.c_int32 * 32)()
    assert hip_lib.spcbpt_abi_struct_sizes(sizes, 32) == 13                   # no new entry
    assert pkg.api.DISPLAY_SOURCES["bloom"] == 4
    assert np.array_equal(pkg.api.bloom_host(ref.seeded_image(7, 5)), pkg.api.bloom_host(ref.seeded_image(7, 5), **ref.DEFAULTS))
    assert hip_lib.spcbpt_bloom_default_params(None) == INVALID


def test_refusals(pkg, hip_lib):
    img = ref.seeded_image(7, 5)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(levels=0), dict(levels=9), dict(levels=-1), dict(strength=-0.01), dict(strength=1.5), dict(strength=nan), dict(spread=0.0),
               dict(spread=4.5), dict(spread=inf), dict(threshold=-1.0), dict(threshold=nan), dict(clamp=0.0), dict(clamp=-1.0), dict(clamp=inf),
               dict(clamp=3.0e19)):
        with pytest.raises(pkg.SpcbptError) as e:
            pkg.api.bloom_host(img, **kw)
        assert f"({INVALID})" in str(e.value), (kw, str(e.value))
    pkg.api.bloom_host(img, levels=8, strength=1.0, spread=4.0, clamp=2.0 ** 64)        # the ends of the ranges are inside
    pkg.api.bloom_host(img, levels=1, strength=0.0, spread=1e-3, threshold=1e30, clamp=1e-30)
    p = pkg.api.bloom_params()
    out = np.zeros((5, 7, 4), np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    assert hip_lib.spcbpt_bloom_host(None, 7, 5, C.byref(p), fp(out)) == INVALID
    assert hip_lib.spcbpt_bloom_host(fp(img), 7, 5, None, fp(out)) == INVALID
    assert hip_lib.spcbpt_bloom_host(fp(img), 7, 5, C.byref(p), None) == INVALID
    assert hip_lib.spcbpt_bloom_host(fp(img), 0, 5, C.byref(p), fp(out)) == INVALID
    assert hip_lib.spcbpt_bloom_host(fp(img), 1 << 15, 1 << 14, C.byref(p), fp(out)) == INVALID    # 2^29 pixels
    with pytest.raises(pkg.SpcbptError):
        pkg.api.bloom_params(radius=3)
    with pytest.raises(pkg.SpcbptError):
        pkg.api.bloom_host(np.zeros((5, 7, 3), np.float32))


# ------------------------------------------------------------------------------------------------------------ memory and arithmetic checks
MAIN = r"""
#include <cmath>
#include <cstdio>
#include <vector>
#include "spcbpt.h"
int main() {
    const int sizes[3][2] = {{1, 1}, {9, 1}, {7, 5}};
    const int levels[3] = {1, 3, 8};
    for (auto& wh : sizes)
        for (int L : levels) {
            const int w = wh[0], h = wh[1];
            std::vector<float> img((size_t)w * h * 4), out((size_t)w * h * 4, -1.0f);
            for (size_t i = 0; i < img.size(); i++) img[i] = std::ldexp(1.0f + (float)((i * 37u) % 11u) / 11.0f, (int)((i * 13u) % 23u) - 10);
            img[1] = NAN;
            img[2] = -3.0f;
            if (w * h > 4) { img[4 * 3 + 2] = INFINITY; img[4 * 4] = 3.0e5f; }
            spcbpt_bloom_params p;
            if (spcbpt_bloom_default_params(&p) != SPCBPT_OK) return 2;
            p.levels = L; p.strength = 0.7f; p.spread = 2.0f; p.threshold = 1.0f;
            if (spcbpt_bloom_host(img.data(), w, h, &p, out.data()) != SPCBPT_OK) return 3;
            if (!std::isnan(out[1])) return 4;
            for (size_t i = 0; i < out.size(); i += 4)
                if (out[i + 3] != img[i + 3]) return 5;
            p.levels = 9;
            if (spcbpt_bloom_host(img.data(), w, h, &p, out.data()) != SPCBPT_ERR_INVALID_ARG) return 6;
        }
    std::puts("bloom_host: clean");
    return 0;
}
"""


def test_host_form_is_clean_under_the_sanitizers(tmp_path):
    """bloom_host.cpp with a main of its own under -fsanitize=address,undefined: a stand-alone program, the 1 x 1, 9 x 1 and 7 x 5 cases at
    L = 1, 3, 8 with a NaN, a negative, a +inf and an above-clamp channel."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the library and this program"
    src = os.path.join(str(tmp_path), "bloom_main.cpp")
    exe = os.path.join(str(tmp_path), "bloom_main")
    with open(src, "w") as f:
        f.write(MAIN)
    csrc = os.path.join(ROOT, "spcbpt-optix7_amd", "csrc")
    cmd = [gxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           src, os.path.join(csrc, "bloom_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and "bloom_host: clean" in p.stdout, p.stdout[-3000:]
