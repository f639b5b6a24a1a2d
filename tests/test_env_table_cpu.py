"""The environment map's sampling table as the product builds it (csrc/env_file.cpp: env_build, accumulated in float as upstream's
envMapCMFBuild) against the float64 definition of tests/env_ref.py, without a GPU: tests/native/env_table_check.cpp is compiled with
g++ around env_file.cpp itself and run on rasters written here.  It also checks that the texture is the row-flipped raster bit for
bit, and env_first_undrawable (the helper spcbpt_set_environment refuses a map by) on hand-made tables.

Measured (scenes.sky_texture(w, h); 7 x 5: random texels in [0.2, 1), one of them 100 times brighter):
    size         texels with probability <= 0    max relative error of a texel's probability    median      max |cmf - float64 cmf|
    7 x 5        0                               5.7e-6                                         5.7e-7      7.2e-8
    64 x 32      0                               2.5e-4                                         2.7e-5      2.2e-6
    512 x 256    0                               1.7e-2                                         1.9e-3      2.7e-5
    1024 x 512   0                               6.4e-2                                         7.7e-3      4.5e-4
    2048 x 1024  0                               2.0e-1                                         3.1e-2      6.6e-3
    4096 x 2048  115 466 (1.4 %), first 3 847 914   1                                           1.1e-1      1.0e-2
The error of a texel's probability is no bias (sampling and pdf read the same table); a texel that can never be drawn is: its light is
lost to next-event estimation.  spcbpt_set_environment therefore refuses a map whose table has such a texel."""
import os
import subprocess

import numpy as np
import pytest

from tests import env_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def odd_sky(w=7, h=5, seed=75):
    """An odd-sized raster (not a power of two, width no multiple of four): random positive texels, one of them 100 times the rest."""
    rng = np.random.default_rng(seed)
    a = np.zeros((h, w, 4), np.float32)
    a[..., :3] = rng.uniform(0.2, 1.0, (h, w, 3))
    a[3, 4, :3] *= 100.0
    return a


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("env_table")
    exe = str(d / "env_table_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "env_table_check.cpp")], check=True)

    def run(raster):
        h, w = raster.shape[:2]
        rp, pp = str(d / "raster.bin"), str(d / "reference.bin")
        np.ascontiguousarray(raster, np.float32).tofile(rp)
        env_ref.table(raster).tofile(pp)
        r = subprocess.run([exe, rp, pp, str(w), str(h)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        print(r.stdout.strip())
        f = r.stdout.split()
        return {f[k]: float(f[k + 1]) for k in range(3, len(f), 2)}
    return run


@pytest.mark.parametrize("size", [(64, 32), (7, 5), (512, 256), (1024, 512), (2048, 1024), (4096, 2048)])
def test_float_table_against_the_float64_definition(checker, pkg, size):
    w, h = size
    s = checker(odd_sky() if size == (7, 5) else pkg.scenes.sky_texture(w, h))
    assert abs(s["last"] - 1.0) <= 1e-6
    assert (s["first"] == -1) == (s["zero"] == 0) and s["first"] == s["first_seen"]      # the helper names the first texel that cannot be drawn
    if w * h <= 64 * 32:
        assert s["max_rel"] <= 1e-3, s                   # four times the 2.5e-4 measured at 64 x 32
    if w * h <= 2048 * 1024:
        assert s["zero"] == 0, s
    else:
        # 4096 x 2048: the float table loses texels (measured 115 466 of 8 388 608), so spcbpt_set_environment refuses the map
        assert s["zero"] > 0 and 0 <= s["first"] < w * h, s
