"""tex_fetch_rgb (csrc/dev_bsdf.h: the bilinear, wrapping RGBA8 fetch behind every textured material) and the linearisation
color_tex_sample stores, against the float64 lookup of tests/env_ref.py through the per-function harness (SPCBPT_UNIT_TEX).  The image
tests and the eye-step chain reach the fetch only at the (u, v) their scenes happen to have: inside [0, 1], on 64 x 64 textures.

Three textures of random bytes: 1 x 1, 3 x 2 (odd, not square) and 64 x 64 (the size of bedroom(tex_size=64)).  Records: random
(u, v) in [-3, 4)^2 and the grid of hand-written edges 0, -0.0, 1, every texel centre and border, +-1000.25 and 1e6.
  * colour: within 1e-6 absolute of the float64 lookup at the coordinate the device forms, x = f32(f32(u W) - 0.5), reproduced in
    numpy float32 (the weights are exact fractions of that coordinate, the texels are <= 1);
  * linearised colour: within 2e-4 relative of float64 t^2.2 of the colour the device returned (device powf against libm: the
    figure of tests/test_gpu_units.py)."""
import numpy as np
import pytest

from tests import env_ref
from tests.test_gpu_units import check

pytestmark = pytest.mark.gpu
TEX = 13                         # SPCBPT_UNIT_TEX
ERR_INVALID_ARG, ERR_STATE = -1, -5


@pytest.fixture(scope="module")
def textured(gpu, pkg):
    rng = np.random.default_rng(31)
    scene = pkg.scenes.simple_room()
    scene.textures = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for w, h in ((1, 1), (3, 2), (64, 64))]
    for k in range(3):
        scene.materials[k]["albedo_tex"] = k + 1
    return pkg.Renderer(scene, 0), scene.textures


def _records(tex_no, w, h, rng, n):
    edges_u = np.concatenate([[0.0, -0.0, 1.0, 1000.25, -1000.25, 1e6], (np.arange(w) + 0.5) / w, np.arange(w + 1) / w])
    edges_v = np.concatenate([[0.0, -0.0, 1.0, 1000.25, -1000.25, 1e6], (np.arange(h) + 0.5) / h, np.arange(h + 1) / h])
    eu, ev = edges_u[rng.integers(0, len(edges_u), 2 * n)], edges_v[rng.integers(0, len(edges_v), 2 * n)]
    gu, gv = np.meshgrid(edges_u[:6], edges_v[:6], indexing="ij")
    ru, rv = rng.uniform(-3, 4, n), rng.uniform(-3, 4, n)
    # random x random, edge x edge (the six special values in every combination, the texel grid drawn), edge x random
    u = np.concatenate([ru, gu.ravel(), eu[:n], eu[n:], rng.uniform(-3, 4, n)])
    v = np.concatenate([rv, gv.ravel(), ev[:n], rng.uniform(-3, 4, n), ev[n:]])
    words = np.zeros((len(u), 3), np.uint32)
    words[:, 0] = tex_no
    words[:, 1:] = np.stack([u, v], 1).astype(np.float32).view(np.uint32)
    return words


@pytest.mark.parametrize("k", [0, 1, 2])
def test_fetch_and_linearisation(textured, k):
    r, textures = textured
    img = textures[k]
    h, w = img.shape[:2]
    words = _records(k + 1, w, h, np.random.default_rng(32 + k), 4096)
    out = r.unit(TEX, words, 6).view(np.float32)
    uv = words[:, 1:].view(np.float32)
    x = ((uv[:, 0] * np.float32(w)).astype(np.float32) - np.float32(0.5)).astype(np.float64)
    y = ((uv[:, 1] * np.float32(h)).astype(np.float32) - np.float32(0.5)).astype(np.float64)
    want = env_ref.bilinear_at(env_ref.rgba8_texture(img), x, y)[:, :3]
    assert np.isfinite(out).all()
    check(f"{w} x {h}: tex_fetch_rgb, absolute", out[:, :3], want, 1e-6, 1.0, scale=1.0)
    lin = out[:, :3].astype(np.float64) ** 2.2
    check(f"{w} x {h}: linearised colour, relative", out[:, 3:6].reshape(-1), lin.reshape(-1), 2e-4, 1.0)
    if w == 1:
        assert np.abs(out[:, :3].astype(np.float64) - img[0, 0, :3] / 255.0).max() <= 1e-6


def test_texture_number_is_checked(textured, pkg):
    r, _ = textured
    rec = np.zeros((1, 3), np.uint32)
    for bad in (0, 4, 0xFFFFFFFF):
        rec[0, 0] = bad
        out = np.zeros((1, 6), np.uint32)
        assert r.lib.spcbpt_debug_unit(r.h, TEX, rec.ctypes.data, 3, out.ctypes.data, 6, 1, None, 0) == ERR_INVALID_ARG
    # the environment ops of the harness need an environment map, and an index inside its table
    for op, nin, nout in ((11, 4, 24), (12, 1, 5)):
        rec, out = np.zeros((1, nin), np.uint32), np.zeros((1, nout), np.uint32)
        assert r.lib.spcbpt_debug_unit(r.h, op, rec.ctypes.data, nin, out.ctypes.data, nout, 1, None, 0) == ERR_STATE
    r2 = pkg.Renderer(pkg.scenes.simple_room(), 0)
    r2.set_environment(pkg.scenes.sky_texture(16, 8))
    rec, out = np.full((1, 1), 16 * 8, np.uint32), np.zeros((1, 5), np.uint32)
    assert r2.lib.spcbpt_debug_unit(r2.h, 12, rec.ctypes.data, 1, out.ctypes.data, 5, 1, None, 0) == ERR_INVALID_ARG
    rec[0, 0] = 16 * 8 - 1
    assert r2.unit(12, rec, 5).view(np.float32)[0, 0] == 1.0       # the last CMF entry
    rec, out = np.zeros((1, 3), np.uint32), np.zeros((1, 6), np.uint32)
    rec[0, 0] = 1
    assert r2.lib.spcbpt_debug_unit(r2.h, TEX, rec.ctypes.data, 3, out.ctypes.data, 6, 1, None, 0) == ERR_INVALID_ARG   # a scene without textures
