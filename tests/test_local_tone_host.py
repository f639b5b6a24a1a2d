"""The local tone stage on the host -- the per-pixel and per-node code the kernels run (csrc/local_tone_pixel.h) behind
spcbpt_local_tone_host -- against the float64 numpy definition of tests/local_tone_ref.py, on synthetic images.  Needs no GPU.

The bar is derived in tests/local_tone_ref.py:  bar_g = (|c - 1| + |d - 1|) (2 2^-13 + (n + 8) 2^-24 16) in the log of the gain,
n = (2 s - 1)^2, and  ln 2 bar_g + 2^-13 + 4 2^-24  relative in an output channel.  That it separates a right result from a wrong one is
checked here too: three mutants of the reference (wz constant, tx and ty swapped in the slice, A without the division by B) miss it.

Measured (the host form against the definition, worst |O - O_ref| / bar over the shapes and parameter sets): 0.09."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import local_tone_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
IDS = [ref.shape_id(s) for s in ref.SHAPES]
BAR_MATH = 2.0 ** -13


@pytest.fixture(scope="module")
def images():
    return {ref.shape_id(s): ref.planted_image(s[0], s[1]) for s in ref.SHAPES}


def _kw(shape, ps):
    return dict(ps, cell=shape[2], range=shape[3])


# ------------------------------------------------------------------------------------------------------------ against the definition
@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_host_form_meets_the_bar(pkg, images, shape):
    img, plants = images[ref.shape_id(shape)]
    worst = 0.0
    for ps in ref.PARAM_SETS:
        kw = _kw(shape, ps)
        out = pkg.api.local_tone_host(img, **kw)
        r = ref.local_tone(img, **kw)
        assert out.dtype == np.float32 and out.shape == img.shape
        no = ref.no_part_mask(plants, img.shape[:2])
        assert np.array_equal(~r["part"], no), kw                                       # who takes part: exactly the others
        assert np.array_equal(out.view(np.uint32)[no], img.view(np.uint32)[no])          # a pixel that takes no part keeps its bits
        assert np.array_equal(out[..., 3].view(np.uint32), img[..., 3].view(np.uint32))  # alpha is the source's
        ratio, n = ref.excess(out, r, **kw)
        print(f"{ref.shape_id(shape)} {ps}: |O - O_ref| / bar {ratio:.4f} over {n} pixels")
        worst = max(worst, ratio)
        assert n == img.shape[0] * img.shape[1] - int(no.sum())
        assert ratio <= 1.0, (shape, kw, ratio)
    print(f"{ref.shape_id(shape)}: worst {worst:.4f}")


@pytest.mark.parametrize("mutant", ref.MUTANTS)
def test_bar_rejects_the_mutants(images, mutant):
    """The reference itself, made wrong in one place, against the right reference: outside the bar on at least one of the images, for
    every parameter set (the images of a few pixels cannot tell every mutant from the definition)."""
    for ps in ref.PARAM_SETS:
        worst = 0.0
        for shape in ref.SHAPES:
            img, _ = images[ref.shape_id(shape)]
            kw = _kw(shape, ps)
            r = ref.local_tone(img, **kw)
            assert ref.excess(r["O"], r, **kw)[0] == 0.0
            worst = max(worst, ref.excess(ref.local_tone(img, mutant=mutant, **kw)["O"], r, **kw)[0])
        print(f"{mutant} {ps}: worst |O_mutant - O_ref| / bar {worst:.3g}")
        assert worst > 1.0, (mutant, ps, worst)


# ------------------------------------------------------------------------------------------------------------ lt_log2 and lt_exp2
def test_log2_is_accurate_and_monotone(pkg):
    """Exhaustive over the octave [1, 2) -- all 2^23 mantissas; e = 0 there, so that lt_log2 is P itself and no coarser sum with e hides a
    step down -- and at the borders of every octave of [2^-16, 2^16]: the power of two, its predecessor and its successor."""
    m = (np.arange(1 << 23, dtype=np.uint32) | np.uint32(0x3F800000)).view(np.float32)
    got = pkg.api.local_tone_math_host(m, 0)
    err = float(np.abs(got.astype(np.float64) - np.log2(m.astype(np.float64))).max())
    print(f"max |lt_log2 - log2| over [1, 2): {err:.3e}")
    assert err <= BAR_MATH
    assert got[0] == 0.0 and (np.diff(got) >= 0).all() and got[-1] <= 1.0
    p = np.float32(2.0) ** np.arange(-16, 17, dtype=np.float32)
    edge = np.unique(np.concatenate([p, np.nextafter(p, np.float32(0))[1:], np.nextafter(p, np.float32(np.inf))[:-1]]))
    got = pkg.api.local_tone_math_host(edge, 0)
    assert np.abs(got.astype(np.float64) - np.log2(edge.astype(np.float64))).max() <= BAR_MATH
    assert (np.diff(got) >= 0).all()
    assert np.array_equal(pkg.api.local_tone_math_host(p, 0), np.arange(-16, 17, dtype=np.float32))   # a power of two: its exponent, exactly


def test_exp2_is_accurate_and_monotone(pkg):
    """A dense grid of g in [-32, 32] (2^21 + 1 points, 3e-5 apart), every integer with its two neighbours, and the octave [0, 1) at
    2^20 points; outside [-32, 32] the argument is clamped."""
    f = np.linspace(0.0, 1.0, (1 << 20) + 1).astype(np.float32)
    ints = np.arange(-32, 33, dtype=np.float32)
    g = np.unique(np.concatenate([np.linspace(-32.0, 32.0, (1 << 21) + 1).astype(np.float32), ints, np.nextafter(ints, np.float32(-np.inf))[1:],
                                  np.nextafter(ints, np.float32(np.inf))[:-1], f, np.float32([-1e-30, 1e-30, -1e-10])]))
    got = pkg.api.local_tone_math_host(g, 1)
    err = float(np.abs(got.astype(np.float64) / 2.0 ** g.astype(np.float64) - 1.0).max())
    print(f"max |lt_exp2 / exp2 - 1| over [-32, 32]: {err:.3e}")
    assert err <= BAR_MATH
    assert (np.diff(got) >= 0).all()
    one = pkg.api.local_tone_math_host(np.float32([0.0, -0.0]), 1)
    assert one.tobytes() == np.float32([1.0, 1.0]).tobytes()
    assert np.array_equal(pkg.api.local_tone_math_host(ints, 1), (2.0 ** ints.astype(np.float64)).astype(np.float32))
    far = pkg.api.local_tone_math_host(np.float32([-1e9, -33.0, 33.0, 1e9, -np.inf, np.inf]), 1)
    assert np.array_equal(far, np.float32([2.0 ** -32, 2.0 ** -32, 2.0 ** 32, 2.0 ** 32, 2.0 ** -32, 2.0 ** 32]))


# ------------------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_unit_slopes_return_the_source(pkg, images, shape):
    img, _ = images[ref.shape_id(shape)]
    for blur in (0, 1, 4):
        out = pkg.api.local_tone_host(img, cell=shape[2], range=shape[3], blur=blur, compress=1.0, detail=1.0, anchor=3.0)
        assert out.tobytes() == img.tobytes(), (shape, blur)


@pytest.mark.parametrize("blur", [0, 1, 4])
def test_a_strong_edge_gets_no_halo(pkg, blur):
    """23 x 37, the left part at L = -4, the right part at L = +8, s = 8, rho = 1, detail 1.  Twelve stops are more than 2 + blur bins, so
    no node holds pixels of both sides: in the definition the base of every pixel is its own L (the condition, checked first), and the
    gain of every pixel, the two columns at the edge included, is the gain a flat image of its side gets.  With wz constant the base is
    off by six stops at the edge."""
    img = ref.edge_image()
    kw = dict(cell=8, range=1.0, blur=blur, compress=0.5, detail=1.0)
    r = ref.local_tone(img, **kw)
    assert np.abs(r["base"] - r["L"]).max() < 1e-12
    off = np.abs(ref.local_tone(img, mutant="flat_wz", **kw)["base"] - r["L"]).max()
    assert 5.0 < off < 7.0, off
    out = pkg.api.local_tone_host(img, **kw).astype(np.float64)
    gain = out[..., :3] / img[..., :3].astype(np.float64)
    La = np.log2(np.float64(np.float32(0.18)))
    want = np.where(np.arange(23) < 11, 2.0 ** (-0.5 * (-4.0 - La)), 2.0 ** (-0.5 * (8.0 - La)))[None, :, None]
    rel = np.abs(gain / want - 1.0)
    print(f"blur {blur}: worst |gain / flat gain - 1| {rel.max():.3e}, at the edge columns {rel[:, 10:12].max():.3e}; bar {ref.bar_rel(8, 0.5, 1.0):.3e}")
    assert rel.max() <= ref.bar_rel(8, 0.5, 1.0)
    assert np.array_equal(out[..., 3], img[..., 3])


@pytest.mark.parametrize("ps", ref.PARAM_SETS, ids=["defaults", "blur0", "blur4"])
def test_flat_image_gets_one_gain(pkg, ps):
    L0 = 3.0
    img = np.ones((23, 37, 4), np.float32)
    img[..., :3] = np.float32(2.0 ** L0)
    p = dict(ref.DEFAULTS, **ps)
    out = pkg.api.local_tone_host(img, **ps).astype(np.float64)
    want = 2.0 ** ((np.float64(np.float32(p["compress"])) - 1.0) * (L0 - np.log2(np.float64(np.float32(p["anchor"])))))
    rel = np.abs(out[..., :3] / img[..., :3] / want - 1.0)
    assert rel.max() <= ref.bar_rel(p["cell"], p["compress"], p["detail"]), (ps, rel.max())


def test_a_pixel_that_takes_no_part_is_absent(pkg, images):
    """What a NaN, an infinity, a zero or a negative pixel holds changes no other pixel: replacing them by other values that take no
    part either leaves every other pixel's bits, and those bits meet the definition evaluated without them (the bar test above)."""
    shape = ref.SHAPES[3]
    img, plants = images[ref.shape_id(shape)]
    no = ref.no_part_mask(plants, img.shape[:2])
    other = img.copy()
    other[no, :3] = np.float32([0.0, -np.inf, np.nan])
    for ps in ref.PARAM_SETS:
        kw = _kw(shape, ps)
        a, b = pkg.api.local_tone_host(img, **kw), pkg.api.local_tone_host(other, **kw)
        assert np.array_equal(a.view(np.uint32)[~no], b.view(np.uint32)[~no])
        assert np.array_equal(b.view(np.uint32)[no], other.view(np.uint32)[no])
        # ... and it is not that nothing depends on anything: a pixel that does take part is seen by its neighbours
        moved = img.copy()
        y, x = plants["huge"][0]
        moved[y, x, :3] *= np.float32(0.001)
        c = pkg.api.local_tone_host(moved, **kw)
        assert (a.view(np.uint32) != c.view(np.uint32)).any(axis=-1).sum() > 1


@pytest.mark.parametrize("shape", ref.SHAPES[3:], ids=IDS[3:])
def test_channels_carry_one_common_factor(pkg, images, shape):
    img, plants = images[ref.shape_id(shape)]
    part = ~ref.no_part_mask(plants, img.shape[:2])
    out = pkg.api.local_tone_host(img, **_kw(shape, ref.PARAM_SETS[1])).astype(np.float64)
    k = out[..., :3][part] / img[..., :3].astype(np.float64)[part]
    assert np.abs(k / k[:, :1] - 1.0).max() <= 2.0 ** -23 * (1 + 2.0 ** -20)                     # one float32 factor, a rounding per channel
    assert np.abs(np.log2(k[:, 0])).max() > 1.0                              # and it does something


# ------------------------------------------------------------------------------------------------------------ the ABI
def test_defaults_struct_size_and_abi_count(pkg, hip_lib):
    p = pkg.api.local_tone_params()
    assert (p.cell, p.range, p.blur, p.compress, p.detail, p.anchor) == (16, 1.0, 1, 0.5, 1.0, np.float32(0.18))
    assert hip_lib.spcbpt_local_tone_params_struct_size() == C.sizeof(pkg.api.LocalToneParams) == 24
    sizes = (C.c_int32 * 32)()
    assert hip_lib.spcbpt_abi_struct_sizes(sizes, 32) == 13                   # no new entry
    assert pkg.api.DISPLAY_SOURCES["local"] == 5
    img = ref.seeded_image(7, 5)
    assert np.array_equal(pkg.api.local_tone_host(img), pkg.api.local_tone_host(img, **ref.DEFAULTS))
    assert hip_lib.spcbpt_local_tone_default_params(None) == INVALID


def test_refusals(pkg, hip_lib):
    img = ref.seeded_image(7, 5)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(cell=3), dict(cell=65), dict(cell=-1), dict(range=0.49), dict(range=8.5), dict(range=nan), dict(blur=-1), dict(blur=5),
               dict(compress=0.0), dict(compress=2.01), dict(compress=inf), dict(detail=-0.1), dict(detail=4.5), dict(detail=nan),
               dict(anchor=0.0), dict(anchor=-1.0), dict(anchor=inf), dict(anchor=nan)):
        with pytest.raises(pkg.SpcbptError) as e:
            pkg.api.local_tone_host(img, **kw)
        assert f"({INVALID})" in str(e.value), (kw, str(e.value))
    pkg.api.local_tone_host(img, cell=4, range=0.5, blur=4, compress=2.0, detail=4.0, anchor=1e30)        # the ends of the ranges are inside
    pkg.api.local_tone_host(img, cell=64, range=8.0, blur=0, compress=1e-3, detail=0.0, anchor=1e-30)
    p = pkg.api.local_tone_params()
    out = np.zeros((5, 7, 4), np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))   # noqa: E731
    assert hip_lib.spcbpt_local_tone_host(None, 7, 5, C.byref(p), fp(out)) == INVALID
    assert hip_lib.spcbpt_local_tone_host(fp(img), 7, 5, None, fp(out)) == INVALID
    assert hip_lib.spcbpt_local_tone_host(fp(img), 7, 5, C.byref(p), None) == INVALID
    assert hip_lib.spcbpt_local_tone_host(fp(img), 0, 5, C.byref(p), fp(out)) == INVALID
    assert hip_lib.spcbpt_local_tone_host(fp(img), 1 << 15, 1 << 14, C.byref(p), fp(out)) == INVALID    # 2^29 pixels
    fine = pkg.api.local_tone_params(cell=4, range=0.5)
    assert hip_lib.spcbpt_local_tone_host(fp(img), 4096, 4096, C.byref(fine), fp(out)) == INVALID        # 1025 x 1025 x 66 nodes > 2^25
    assert hip_lib.spcbpt_local_tone_math_host(None, 1, 0, fp(out)) == INVALID
    assert hip_lib.spcbpt_local_tone_math_host(fp(img), 1, 2, fp(out)) == INVALID
    with pytest.raises(pkg.SpcbptError):
        pkg.api.local_tone_params(radius=3)
    with pytest.raises(pkg.SpcbptError):
        pkg.api.local_tone_host(np.zeros((5, 7, 3), np.float32))


# ------------------------------------------------------------------------------------------------------------ memory and arithmetic checks
MAIN = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "spcbpt.h"
int main() {
    const int cases[5][4] = {{1, 1, 16, 1}, {9, 1, 4, 0}, {1, 9, 4, 4}, {37, 23, 8, 1}, {5, 3, 64, 2}};   // width, height, cell, blur
    const float ranges[3] = {0.5f, 1.0f, 8.0f};
    for (auto& q : cases)
        for (float range : ranges) {
            const int w = q[0], h = q[1];
            std::vector<float> img((size_t)w * h * 4), out((size_t)w * h * 4, -1.0f);
            for (size_t i = 0; i < img.size(); i++) img[i] = std::ldexp(1.0f + (float)((i * 37u) % 11u) / 11.0f, (int)((i * 13u) % 23u) - 10);
            if (w * h > 4) {
                img[1] = NAN;
                img[4 * 2 + 2] = INFINITY;
                img[4 * 3] = -INFINITY;
                img[4 * 4] = img[4 * 4 + 1] = img[4 * 4 + 2] = 0.0f;
            }
            spcbpt_local_tone_params p;
            if (spcbpt_local_tone_default_params(&p) != SPCBPT_OK) return 2;
            p.cell = q[2]; p.blur = q[3]; p.range = range; p.compress = 0.4f; p.detail = 1.3f;
            if (spcbpt_local_tone_host(img.data(), w, h, &p, out.data()) != SPCBPT_OK) return 3;
            if (w * h > 4 && (!std::isnan(out[1]) || std::memcmp(&out[4 * 2], &img[4 * 2], 48) != 0)) return 4;
            for (size_t i = 0; i < out.size(); i += 4)
                if (out[i + 3] != img[i + 3]) return 5;
            p.cell = 65;
            if (spcbpt_local_tone_host(img.data(), w, h, &p, out.data()) != SPCBPT_ERR_INVALID_ARG) return 6;
        }
    const float g[6] = {0.0f, -1e-10f, 32.0f, -40.0f, NAN, 0.5f};
    float e[6], l[6];
    if (spcbpt_local_tone_math_host(g, 6, 1, e) != SPCBPT_OK || e[0] != 1.0f) return 7;
    if (spcbpt_local_tone_math_host(e, 6, 0, l) != SPCBPT_OK || l[0] != 0.0f) return 8;
    std::puts("local_tone_host: clean");
    return 0;
}
"""


def test_host_form_is_clean_under_the_sanitizers(tmp_path):
    """local_tone_host.cpp with a main of its own under -fsanitize=address,undefined: a stand-alone program, five shapes (a footprint cut
    by every image edge, the image inside one cell) at three ranges with a NaN, both infinities and a zero pixel."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build the library and this program"
    src = os.path.join(str(tmp_path), "local_tone_main.cpp")
    exe = os.path.join(str(tmp_path), "local_tone_main")
    with open(src, "w") as f:
        f.write(MAIN)
    csrc = os.path.join(ROOT, "spcbpt-optix7_amd", "csrc")
    cmd = [gxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
           src, os.path.join(csrc, "local_tone_host.cpp"), "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert p.returncode == 0 and "local_tone_host: clean" in p.stdout, p.stdout[-3000:]
