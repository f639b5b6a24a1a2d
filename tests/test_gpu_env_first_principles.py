"""The environment map on the GPU against float64 definitions (tests/env_ref.py), function by function through the per-function
harness (csrc/unit.hip: SPCBPT_UNIT_ENV, SPCBPT_UNIT_ENV_TABLE): dir2uv, env_color, env_pdf, env_label, env_sample, env_light_sample
and the tables spcbpt_set_environment uploads.  The other environment tests hold this code to the oracle (the same author's
restatement of the same unfinished upstream feature) and to itself (estimator against estimator, where a wrong scale, flip or
solid-angle factor cancels); here nothing the device code computes is on the reference side.

Two contexts on scenes.courtyard() with its quad light (n_lights = 2): the scene's own 64 x 32 sky, and a 7 x 5 sky of random
positive texels with one texel 100 times the rest (odd, no power of two, width no multiple of four).

Bars (measured values: the docstring of each test):
  * (u, v): UV_BOUND = four times the largest error measured against float64, and no more than 1e-5;
  * colour against the float64 bilinear lookup at the device's own (u, v): 1e-6 x the largest of the four texels (four products and
    three sums in FP32): the filter, the wrap and the flip alone;
  * colour against float64 at the float64 (u, v): UV_BOUND x the local contrast + the term above.  Local contrast = W gx + H gy with
    gx, gy the LARGER of the two opposite edge differences of the bilinear cell: d colour / dx = (1 - ay)(t10 - t00) + ay (t11 - t01)
    is bounded by the larger edge, not by the edge at t00 alone (next to the 7 x 5 map's bright texel that edge is 1 % of the other);
  * pdf within 1e-3 (the table's bar), label exact, both away from texel / cell borders (1e-4 of a texel; at most 1 % left out);
  * chi^2 tests: tail probability above 1e-6 (tests/test_gpu_mesh_light.py: _chi2_sf, _pearson).  The helper's closed form overflows
    beyond ~1300 degrees of freedom, so the 2048 texels of the 64 x 32 map are tested as two halves."""
import math
import re
import time

import numpy as np
import pytest

from tests import env_ref
from tests.test_env_table_cpu import odd_sky
from tests.test_gpu_mesh_light import _chi2_sf, _pearson, _rnd
from tests.test_gpu_units import frac

pytestmark = pytest.mark.gpu
ENV, ENV_TABLE = 11, 12          # SPCBPT_UNIT_ENV, SPCBPT_UNIT_ENV_TABLE
N = 16384
CAM = dict(eye=(0.0, 2.6, 2.6), lookat=(0.0, 0.2, 0.0), up=(0, 1, 0), fov=40.0)
UP_CAM = dict(eye=(0.0, 2.0, 0.0), lookat=(0.0, 10.0, 0.0), up=(0, 0, -1), fov=40.0)   # tests/test_gpu_env_sky_seen.py
UV_MEASURED = 1.19e-7            # the largest |u - u64|, |v - v64| of test_uv_of_random_directions on the MI355X
UV_BOUND = min(4 * UV_MEASURED, 1e-5)
BORDER = 1e-4
DIV_LEVEL = 10                   # the sky's cells per axis; the worlds fixture holds it to the product's constant
LENGTH_ERROR = 8e-7              # |dir| - 1 of an unnormalised specular reflection (FP32 emulation of 2 dot(V, h) h - V)
MAPS = ["sky 64x32", "odd 7x5"]


def _q(name, e):
    q = np.quantile(e, [0.5, 0.9, 0.99, 0.999, 1.0]) if len(e) else np.zeros(5)
    print(f"{name}: error quantiles 50/90/99/99.9/100 % = " + " ".join(f"{x:.3g}" for x in q))
    return float(q[-1])


def _env(r, dirs, seeds=None):
    n = len(dirs)
    words = np.zeros((n, 4), np.uint32)
    words[:, :3] = np.ascontiguousarray(dirs, np.float32).view(np.uint32)
    if seeds is not None:
        words[:, 3] = seeds
    o = r.unit(ENV, words, 24)
    f = o.view(np.float32)
    return dict(u=f[:, 0], v=f[:, 1], color=f[:, 2:5], pdf=f[:, 5], label=o[:, 6].astype(np.int32).astype(np.int64), sdir=f[:, 7:10], sseed=o[:, 10],
                pos=f[:, 11:14], emission=f[:, 14:17], normal=f[:, 17:20], lpdf=f[:, 20], sub=o[:, 21].astype(np.int32).astype(np.int64),
                dir_pos_pdf=f[:, 22], lseed=o[:, 23])


def _unit_dirs(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


@pytest.fixture(scope="module")
def worlds(gpu, pkg):
    scene = pkg.scenes.courtyard()
    env = scene.environment
    out = {}
    for name, raster in zip(MAPS, (env["rgba"], odd_sky())):
        r = pkg.Renderer(scene, 0)
        r.set_camera_lookat(CAM["eye"], CAM["lookat"], CAM["up"], CAM["fov"], 1.0)
        r.resize(64, 64)
        r.set_environment(raster, env["center"], env["radius"])
        r.set_light_trace(2000, 64, 1)
        r.set_subspace()
        e = r.environment()
        h, w = raster.shape[:2]
        assert (e["width"], e["height"], e["n_lights"]) == (w, h, 2)
        # Context::set_environment: div_level = (int)sqrt(0.5 * SPCBPT_NUM_SUBSPACE_LIGHTSOURCE)
        assert DIV_LEVEL == int(math.sqrt(0.5 * pkg.api.NUM_SUBSPACE_LIGHTSOURCE)) and env_ref.NUM_SUBSPACE == pkg.api.NUM_SUBSPACE
        t = r.unit(ENV_TABLE, np.arange(w * h, dtype=np.uint32).reshape(-1, 1), 5).view(np.float32)
        p64 = env_ref.table(raster)
        c64 = np.cumsum(p64)
        cmf = t[:, 0].copy()
        out[name] = dict(r=r, raster=raster, w=w, h=h, center=np.asarray(env["center"], np.float64), radius=float(e["radius"]), cmf=cmf,
                         tex=t[:, 1:5].reshape(h, w, 4).copy(), p64=p64, c64=c64, eps=float(np.abs(cmf.astype(np.float64) - c64).max()) + 2.0 ** -24,
                         tex64=env_ref.texture(raster))
    return out


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("name", MAPS)
def test_tables(worlds, name):
    """The uploaded texture is the row-flipped raster bit for bit (alpha 1); the CMF is non-decreasing, ends at 1 within 1e-6, and a
    texel's probability (the float difference env_pdf takes) is the float64 definition's within 1e-3 -- four times the 2.5e-4 of the
    CPU build of the 64 x 32 table.  Measured on the MI355X (the tables are built on the host: the CPU figures): 64 x 32 max 2.5e-4,
    max |cmf - float64 cmf| 2.2e-6; 7 x 5 max 5.7e-6, 7.2e-8."""
    t = worlds[name]
    flipped = np.ascontiguousarray(t["raster"][::-1, :, :3], np.float32)
    assert np.array_equal(t["tex"][..., :3].view(np.uint32), flipped.view(np.uint32))
    assert (t["tex"][..., 3] == 1.0).all()
    cmf = t["cmf"]
    assert (np.diff(cmf) >= 0).all() and abs(float(cmf[-1]) - 1.0) <= 1e-6
    p = np.diff(cmf, prepend=np.float32(0.0)).astype(np.float64)        # float32 differences, as env_pdf takes them
    worst = _q(f"{name}: texel probability, relative", np.abs(p - t["p64"]) / t["p64"])
    print(f"{name}: max |cmf - float64 cmf| = {t['eps'] - 2.0 ** -24:.3g}")
    assert worst <= 1e-3


# ---------------------------------------------------------------------------------------------------------------- 2
def _uv_error(o, d):
    u64, v64 = env_ref.dir2uv(d.astype(np.float64))
    du = np.abs(o["u"].astype(np.float64) - u64)
    return np.maximum(np.minimum(du, 1.0 - du), np.abs(o["v"].astype(np.float64) - v64))


def test_uv_of_random_directions(worlds):
    """dir2uv (atan2f, acosf, sinf) of random unit directions against float64: the largest error of u or v, asserted at four times
    the value measured and at most 1e-5 (6e-4 of a texel at 64 texels).  Measured on the MI355X: 1.19e-7 at most (median 3.0e-8,
    99.9 % 8.9e-8), so the bar is 4.76e-7."""
    rng = np.random.default_rng(21)
    d = _unit_dirs(rng, N)
    o = _env(worlds[MAPS[0]]["r"], d)
    worst = _q("(u, v) against float64", _uv_error(o, d))
    assert np.isfinite(o["u"]).all() and np.isfinite(o["v"]).all()
    assert UV_BOUND <= 1e-5 and worst <= UV_BOUND, (worst, UV_BOUND)


# ---------------------------------------------------------------------------------------------------------------- 3
def _color_bars(t, o, d, uv_bound):
    """(error / bar) of part (a) and of part (b) for the ENV records o of the directions d"""
    got = o["color"].astype(np.float64)
    contrast, big = env_ref.local_contrast(t["tex64"], *env_ref.dir2uv(d.astype(np.float64)))
    # (the cell the float64 (u, v) lies in and the device's differ when a texel centre lies between them: the larger scale of the two)
    contrast_dev, big_dev = env_ref.local_contrast(t["tex64"], o["u"].astype(np.float64), o["v"].astype(np.float64))
    ea = np.abs(got - env_ref.bilinear(t["tex64"], o["u"].astype(np.float64), o["v"].astype(np.float64))[..., :3]).max(-1)
    eb = np.abs(got - env_ref.env_color(t["raster"], d.astype(np.float64))).max(-1)
    return ea / (1e-6 * big_dev), eb / (uv_bound * np.maximum(contrast, contrast_dev) + 1e-6 * np.maximum(big, big_dev)), ea, eb


@pytest.mark.parametrize("name", MAPS)
def test_env_color(worlds, name):
    """(a) the filter, the wrap and the flip: against the float64 bilinear lookup at the device's own (u, v); (b) against float64 all
    the way.  Bars: the module docstring.  Measured on the MI355X, largest share of the bar: (a) 0.18 (64 x 32), 0.32 (7 x 5);
    (b) 0.16, 0.14 (absolute 1.1e-4 next to the sun, 7.0e-5 next to the bright texel)."""
    t = worlds[name]
    d = _unit_dirs(np.random.default_rng(22), N)
    o = _env(t["r"], d)
    ra, rb, ea, eb = _color_bars(t, o, d, UV_BOUND)
    _q(f"{name}: colour at the device's (u, v), absolute", ea)
    _q(f"{name}: colour at the device's (u, v), share of the bar", ra)
    _q(f"{name}: colour against float64, absolute", eb)
    _q(f"{name}: colour against float64, share of the bar", rb)
    assert ra.max() <= 1.0 and rb.max() <= 1.0


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("name", MAPS)
def test_env_pdf_and_label(worlds, name):
    """env_pdf within 1e-3 of p_i size / 4 pi, env_label exact, for the directions whose float64 texel / cell coordinate is not within
    1e-4 of an integer (at most 1 % are; random directions: about 0.04 %)."""
    t = worlds[name]
    d = _unit_dirs(np.random.default_rng(23), N)
    o = _env(t["r"], d)
    pdf64, edge_p = env_ref.env_pdf(t["raster"], d.astype(np.float64))
    lab64, edge_l = env_ref.env_label(d.astype(np.float64), DIV_LEVEL)
    keep_p, keep_l = edge_p > BORDER, edge_l > BORDER
    print(f"{name}: left out at a border: pdf {1 - frac(keep_p):.5f}, label {1 - frac(keep_l):.5f}")
    assert frac(keep_p) >= 0.99 and frac(keep_l) >= 0.99
    worst = _q(f"{name}: pdf, relative", np.abs(o["pdf"][keep_p].astype(np.float64) - pdf64[keep_p]) / pdf64[keep_p])
    assert worst <= 1e-3
    assert np.array_equal(o["label"][keep_l], lab64[keep_l])
    assert ((o["label"] >= 900) & (o["label"] <= 999)).all()


# ---------------------------------------------------------------------------------------------------------------- 5
def _edge_directions(w, h):
    f = np.float32
    d = [(0, 1, 0), (0, -1, 0), (1, 0, 0), (-1, 0, 0), (0, 0, 1), (0, 0, -1)]
    for y in (0.3, -0.7, 0.0):                              # the u seam: x = +0 and -0, z < 0
        z = -math.sqrt(1 - y * y)
        d += [(0.0, y, z), (-0.0, y, z)]
    u_c, u_e = (np.arange(w) + 0.5) / w, np.arange(w + 1) / w
    for v in (0.5 / h, (h - 0.5) / h):                      # texel centres of row 0 and row h - 1
        d += [tuple(x) for x in env_ref.uv2dir(u_c, np.full(w, v))]
    for v in (1.0 / h, (h - 1.0) / h):                      # their inner corners (the outer ones are the poles, above)
        d += [tuple(x) for x in env_ref.uv2dir(u_e, np.full(w + 1, v))]
    base = np.array(d, f)
    scaled = [base, base * f(1 + LENGTH_ERROR), base * f(1 - LENGTH_ERROR)]
    return np.concatenate(scaled), len(base)


def _candidates(d64, w, h, table_or_none, div):
    """The values the texels / cells within BORDER of the float64 (u, v) of d64 hold: (n, 4)"""
    u, v = env_ref.dir2uv(d64)
    out = []
    for su in (-1, 1):
        for sv in (-1, 1):
            if table_or_none is not None:
                uu, vv = np.mod(u + su * BORDER / w, 1.0), np.clip(v + sv * BORDER / h, 0.0, 1.0)
                i, _ = env_ref.texel_of(uu, vv, w, h)
                out.append(table_or_none[i] * (w * h) / (4 * np.pi))
            else:
                uu, vv = np.mod(u + su * BORDER / div, 1.0), np.clip(v + sv * BORDER / div, 0.0, 1.0)
                ux, uy = np.clip(np.floor(uu * div), 0, div - 1), np.clip(np.floor(vv * div), 0, div - 1)
                out.append(env_ref.NUM_SUBSPACE - 1 - (ux * div + uy))
    return np.stack(out, 1)


@pytest.mark.parametrize("name", MAPS)
def test_edge_directions(worlds, name):
    """Hand-written directions: the poles, the six axes, the u seam (x = +0 / -0, z < 0), texel centres and corners of the first and
    the last row -- and each of them scaled by 1 +- 8e-7, the length error of a specular reflection that bsdf_sample does not
    renormalise (|y| reaches 1.0000008).  Every output is finite; colour, pdf and label are those of the direction rescaled to unit
    length: the colour under the bar of test_env_color with the (u, v) bound widened by the length error's own share (v = (1 + y) / 2
    moves by 4e-7 |y|), pdf (1e-3) and label (exact) those of a texel / cell within 1e-4 of the float64 (u, v); and, device against
    device, pdf and label of a scaled record are those of its unit-length record bit for bit unless the direction sits on a border
    (64 x 32: 130 / 254 of the 270 directions are off a texel / cell border; 7 x 5: 19 / 2 of 42 -- its rows end on cell borders).
    Before dir2uv clamped dir.y, the MI355X returned for the two records of each map with |y| > 1 (the poles scaled by 1 + 8e-7):
    u 0.5, v NaN, colour (NaN, NaN, NaN), the pdf of a texel of row 0 and label 949 (cell row 0) at BOTH poles; every other record
    passed.  With the clamp the same records return the pole's own values (largest share of the colour bar 0.43 / 0.22)."""
    t = worlds[name]
    d, nb = _edge_directions(t["w"], t["h"])
    o = _env(t["r"], d)
    bad = ~(np.isfinite(o["u"]) & np.isfinite(o["v"]) & np.isfinite(o["color"]).all(1) & np.isfinite(o["pdf"]))
    if bad.any():
        k = np.nonzero(bad)[0]
        print(f"{name}: {len(k)} records with a non-finite output, e.g. direction {d[k[0]]!r}: u {o['u'][k[0]]} v {o['v'][k[0]]} colour {o['color'][k[0]]} "
              f"pdf {o['pdf'][k[0]]} label {o['label'][k[0]]}; |y| > 1 in {int((np.abs(d[k, 1]) > 1).sum())} of them")
    assert not bad.any(), d[bad]
    d64 = d.astype(np.float64)
    d64 /= np.linalg.norm(d64, axis=1, keepdims=True)
    _, rb, _, eb = _color_bars(t, o, d64, UV_BOUND + 0.5 * 1.05 * LENGTH_ERROR)
    _q(f"{name}: edge colours against float64 of the unit direction, share of the bar", rb)
    assert rb.max() <= 1.0
    cand = _candidates(d64, t["w"], t["h"], t["p64"], DIV_LEVEL)
    ok = (np.abs(o["pdf"].astype(np.float64)[:, None] - cand) <= 1e-3 * cand).any(1)
    assert ok.all(), (d[~ok], o["pdf"][~ok])
    cand = _candidates(d64, t["w"], t["h"], None, DIV_LEVEL)
    ok = (o["label"][:, None] == cand).any(1)
    assert ok.all(), (d[~ok], o["label"][~ok])
    assert o["label"][0] % 10 == 0 and o["label"][1] % 10 == 9          # uy = 9 at +y, 0 at -y: 999 - (ux 10 + uy)
    # the device against itself: away from a border (the corners and the seam sit on one by construction) a scaled record returns the
    # pdf and the label of its unit-length record bit for bit
    _, edge_p = env_ref.env_pdf(t["raster"], d64[:nb])
    _, edge_l = env_ref.env_label(d64[:nb], DIV_LEVEL)
    poles = np.abs(d64[:nb, 1]) == 1.0                                  # v = 0 or 1 is a border by the letter, but the clamp decides it
    for k in (1, 2):
        sel = (edge_p > BORDER) | poles
        assert np.array_equal(o["pdf"][k * nb:(k + 1) * nb][sel].view(np.uint32), o["pdf"][:nb][sel].view(np.uint32))
        sel = (edge_l > BORDER) | poles
        assert np.array_equal(o["label"][k * nb:(k + 1) * nb][sel], o["label"][:nb][sel])
    print(f"{name}: {nb} hand-written directions, {int(((edge_p > BORDER) | poles).sum())} / {int(((edge_l > BORDER) | poles).sum())} of them off a texel / cell border")


# ---------------------------------------------------------------------------------------------------------------- 6
def _lcg(seed, times):
    s = seed.copy()
    for _ in range(times):
        s, _r = _rnd(s)
    return s


@pytest.mark.parametrize("name", MAPS)
def test_env_sample(worlds, name):
    """2^18 seeds (measured: eps 2.3e-6 / 1.3e-7, 0.04 % of the samples at a border, tail probabilities 0.26 ... 0.61).  The seed after
    is the LCG applied three times.  The texel a sample lands in (from the float64 (u, v) of the returned
    direction; samples within 1e-4 of a border left out, at most 1 %) is the one whose float64 CMF interval holds the first random
    number: C64[l - 1] - eps <= rnd0 <= C64[l] + eps, eps = the largest |device cmf - float64 cmf| + one ulp (an off-by-one of the
    bisection fails this for almost every sample; a histogram would forgive it on a smooth map).  Texel counts against p_i and the
    8 x 8 histogram of the in-texel position against uniform: chi^2 tail probabilities above 1e-6 (64 x 32: each half of the texels
    within itself, and the two halves' totals against each other)."""
    t = worlds[name]
    w, h, n = t["w"], t["h"], 1 << 18
    rng = np.random.default_rng(26)
    seeds = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    o = _env(t["r"], np.tile(np.array([[0, 1, 0]], np.float32), (n, 1)), seeds)
    assert np.array_equal(o["sseed"], _lcg(seeds, 3))
    _, rnd0 = _rnd(seeds)
    rnd0 = rnd0.astype(np.float64)
    sd = o["sdir"].astype(np.float64)
    assert np.isfinite(sd).all() and np.abs(np.linalg.norm(sd, axis=1) - 1).max() <= 1e-6
    u, v = env_ref.dir2uv(sd)
    l, edge = env_ref.texel_of(u, v, w, h)
    keep = edge > BORDER
    print(f"{name}: samples left out at a texel border {1 - frac(keep):.5f}; eps {t['eps']:.3g}")
    assert frac(keep) >= 0.99
    lo = np.concatenate([[0.0], t["c64"]])[l]
    hi = t["c64"][l]
    inside = (lo - t["eps"] <= rnd0) & (rnd0 <= hi + t["eps"])
    assert inside[keep].all(), (int((~inside[keep]).sum()), l[keep & ~inside][:8], rnd0[keep & ~inside][:8])
    counts = np.bincount(l, minlength=w * h)
    expected = t["p64"] * n
    if name == MAPS[0]:
        assert expected.min() >= 32 * (1 - 1e-9)
    halves = [slice(None)] if w * h <= 1024 else [slice(0, w * h // 2), slice(w * h // 2, None)]
    for s in halves:
        e = expected[s] * counts[s].sum() / expected[s].sum()
        chi2, df = _pearson(counts[s], e)
        p = _chi2_sf(chi2, df)
        print(f"{name}: texel counts: chi^2 = {chi2:.1f} with {df} degrees of freedom (tail probability {p:.3g})")
        assert p > 1e-6, (chi2, df)
    if len(halves) > 1:                                                  # and the split of the mass between the halves
        tot = np.array([counts[s].sum() for s in halves])
        chi2, df = _pearson(tot, np.array([expected[s].sum() for s in halves]))
        p = _chi2_sf(chi2, df)
        print(f"{name}: samples per half: chi^2 = {chi2:.2f} with {df} degree of freedom (tail probability {p:.3g})")
        assert p > 1e-6, (chi2, df)
    fx, fy = u * w - np.floor(u * w), v * h - np.floor(v * h)
    hist = np.bincount(np.minimum((fx * 8).astype(int), 7) * 8 + np.minimum((fy * 8).astype(int), 7), minlength=64)
    chi2, df = _pearson(hist, np.full(64, n / 64.0))
    p = _chi2_sf(chi2, df)
    print(f"{name}: in-texel position: chi^2 = {chi2:.1f} with {df} degrees of freedom (tail probability {p:.3g})")
    assert p > 1e-6, (chi2, df)


# ---------------------------------------------------------------------------------------------------------------- 7
def _onb(n):
    """Any orthonormal frame that depends on the direction alone shows whether the angle on the disk is uniform (Onb's)."""
    b = np.where((np.abs(n[:, 0]) > np.abs(n[:, 2]))[:, None], np.stack([-n[:, 1], n[:, 0], np.zeros(len(n))], 1), np.stack([np.zeros(len(n)), -n[:, 2], n[:, 1]], 1))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    return np.cross(b, n), b


@pytest.mark.parametrize("name", MAPS)
def test_env_light_sample(worlds, name):
    """What a light sub-path that starts on the sky carries: normal = minus the direction and emission, pdf x n_lights, subspace = the
    op's own env_color / env_pdf / env_label of that direction, all bit for bit; the seed after = five LCG steps; dir_pos_pdf =
    1 / (pi r^2) to 1e-6; the origin on the disk of radius r around c + 10 r d, normal d: off the plane by at most 1e-5 r (a few ulps
    of 10 r), at most r (1 + 1e-5) from the axis; uniform on it (rho^2 / r^2 and the angle: chi^2 with 16 bins each, and 4 x 4 jointly)."""
    t = worlds[name]
    r, c, R = t["r"], t["center"], t["radius"]
    rng = np.random.default_rng(27)
    seeds = rng.integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
    o = _env(r, np.tile(np.array([[0, 1, 0]], np.float32), (N, 1)), seeds)
    d32 = o["sdir"].copy()
    assert np.array_equal(o["normal"].view(np.uint32), (-d32).view(np.uint32))
    o2 = _env(r, d32)
    assert np.array_equal(o["emission"].view(np.uint32), o2["color"].view(np.uint32))
    assert np.array_equal((o["lpdf"] * np.float32(2.0)).view(np.uint32), o2["pdf"].view(np.uint32))
    assert np.array_equal(o["sub"], o2["label"])
    assert np.array_equal(o["lseed"], _lcg(seeds, 5))
    want = 1.0 / (np.pi * R * R)
    assert np.abs(o["dir_pos_pdf"].astype(np.float64) - want).max() <= 1e-6 * want
    d = d32.astype(np.float64)
    off = o["pos"].astype(np.float64) - c[None, :] - 10 * R * d
    along = (off * d).sum(1)
    q = off - along[:, None] * d
    rho = np.linalg.norm(q, axis=1)
    _q(f"{name}: origin off the disk's plane / r", np.abs(along) / R)
    print(f"{name}: largest distance from the axis / r = {rho.max() / R:.7f}")
    assert np.abs(along).max() <= 1e-5 * R and rho.max() <= R * (1 + 1e-5)
    tt, bb = _onb(d)
    a = np.clip((rho / R) ** 2, 0, 1 - 1e-12)
    ang = (np.arctan2((q * bb).sum(1), (q * tt).sum(1)) / (2 * np.pi)) % 1.0
    for label, idx, cells in (("rho^2 / r^2", (a * 16).astype(int), 16), ("angle", np.minimum((ang * 16).astype(int), 15), 16),
                              ("jointly", (a * 4).astype(int) * 4 + np.minimum((ang * 4).astype(int), 3), 16)):
        chi2, df = _pearson(np.bincount(idx, minlength=cells), np.full(cells, N / cells))
        p = _chi2_sf(chi2, df)
        print(f"{name}: disk {label}: chi^2 = {chi2:.1f} with {df} degrees of freedom (tail probability {p:.3g})")
        assert p > 1e-6, (label, chi2, df)


# ---------------------------------------------------------------------------------------------------------------- 8
FLOOR_MAT = dict(color=(0.7, 0.68, 0.62), roughness=0.6, metallic=0.0)
FLOOR_CAM = dict(eye=(0.0, 6.0, 0.0), lookat=(0.0, 0.0, 0.0), up=(0, 0, -1), fov=40.0)


def _floor_sky(w=32, h=16):
    """Raster (row 0 = the zenith): a vertical gradient over a dimmer ground half, a left-right asymmetry, a mild sun (luminance about
    8) some 35 degrees above the horizon."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    u, v = (x + 0.5) / w, (y + 0.5) / h
    lum = np.where(v < 0.5, 0.8 + 0.5 * np.clip(1 - 2 * v, 0, 1), 0.45) * (1 + 0.3 * np.sin(2 * np.pi * u))
    rgb = lum[..., None] * np.array([0.8, 0.95, 1.25])
    d2 = ((u - 0.3) * 2) ** 2 + (v - 0.22) ** 2
    rgb = rgb + (8.0 / 3) * np.exp(-d2 / (2 * 0.06 ** 2))[..., None] * np.array([1.1, 1.0, 0.9])
    return np.concatenate([rgb, np.zeros((h, w, 1))], -1).astype(np.float32)


def _sky_nodes(w, h, k):
    """(u, v) of the 2 x 2 Gauss-Legendre points of every k x k sub-cell of the texels of the upper hemisphere (v >= 1 / 2: a texel
    border for even h).  With k even a sub-cell lies inside one bilinear patch (they end at the texel centres), where the integrand is
    smooth.  Equal (u, v) area is equal solid angle: every node weighs 2 pi / count."""
    gp = np.array([-1.0, 1.0]) / math.sqrt(3) * 0.5 + 0.5
    nu, nv = w * k, (h // 2) * k
    us = (np.arange(nu)[:, None] + gp[None, :]).reshape(-1) / nu
    vs = 0.5 + 0.5 * (np.arange(nv)[:, None] + gp[None, :]).reshape(-1) / nv
    U, V = np.meshgrid(us, vs, indexing="ij")
    return U.ravel(), V.ravel()


def _sky_radiance(ob, raster, wo, k, chunk=512):
    """Float64 radiance (m, 3) a horizontal floor (normal +y) sends towards wo under the sky `raster`: the integral over the upper
    hemisphere of env_color64(w) f(wo, w) cos(theta) dw, f from the oracle's BSDF evaluator (tests/test_gpu_units.py pins it), as
    _direct_light of tests/test_gpu_mesh_light.py."""
    h, w = raster.shape[:2]
    U, V = _sky_nodes(w, h, k)
    wi = env_ref.uv2dir(U, V)
    wt = env_ref.bilinear(env_ref.texture(raster), U, V)[:, :3] * wi[:, 1:2] * (2 * np.pi / len(U))
    wi32 = wi.astype(np.float32)
    out = np.zeros((len(wo), 3))
    for s in range(0, len(wo), chunk):
        ws = wo[s:s + chunk].astype(np.float32)
        nvl = np.empty((len(ws), len(wi), 9), np.float32)
        nvl[..., 0:3] = np.array([0, 1, 0], np.float32)
        nvl[..., 3:6] = ws[:, None, :]
        nvl[..., 6:9] = wi32[None, :, :]
        f, _ = ob.bsdf_eval_pdf(FLOOR_MAT, nvl.reshape(-1, 9))
        out[s:s + chunk] = np.einsum("ijc,jc->ic", f.reshape(len(ws), len(wi), 3).astype(np.float64), wt)
    return out


def test_lit_floor_against_quadrature(gpu, pkg, ob):
    """The radiometric scale.  An 8 x 8 floor alone under a 32 x 16 sky, a quad light below it that faces down (it lights nothing and
    keeps n_lights = 2 in the estimator), the camera above with every pixel on the floor: a plane does not see itself, so "pt" renders
    the direct sky light, by next-event estimation only.  Truth per pixel: the quadrature of _sky_radiance, sub-cells halved until no
    value of a probe moves by 1e-5.  The radiance is evaluated at the pixel centres; that the mean over 4 x 4 positions of a pixel is
    the centre's value to 1e-6 is asserted on the probe (measured 5e-8: sixteen times the reference for nothing).
    Measured on the MI355X: 2 x 2 -> 4 x 4 sub-cells move the radiance by 5.2e-7; 640 frames, image mean / quadrature 0.99843 with a
    standard error of 1.64e-3, every block inside its bar (largest |z| 2.7); image mean / flipped truth 2.46.  The whole test takes
    1.4 s there (the host quadrature, 17 M BSDF evaluations by the oracle, included); the sub-cell count is settled on the probe's 64
    pixels, as the mesh-light test settles its level on a sample.
    Bars of test_direct_light_against_quadrature: image mean within 0.5 % with its standard error below a third of that (frames are
    added in batches of 128 until it is, 2048 at most), >= 99 % of the 8 x 8 blocks within 4 s + 0.5 %.  With the raster turned upside
    down in the truth the image mean must MISS its bar: the test sees the row flip."""
    from tests.denoise_ref import pixel_centre_dirs
    from tests.test_gpu_mesh_light import _lum
    S = 64
    b = pkg.scenes._Builder()
    b.grid((-4, 0, 4), (8, 0, 0), (0, 0, -8), 2, 2, 0)                      # normal +y
    lights = [dict(position=(-0.25, -1.0, -0.25), u=(0.5, 0, 0), v=(0, 0, 0.5), emission=(1, 1, 1), div_level=1)]   # normal -y
    scene = b.finish([FLOOR_MAT], lights, camera=FLOOR_CAM, name="floor")
    raster = _floor_sky()
    r = pkg.Renderer(scene, 0)
    U, V, W = pkg.camera_frame(FLOOR_CAM["eye"], FLOOR_CAM["lookat"], FLOOR_CAM["up"], FLOOR_CAM["fov"], 1.0)
    r.set_camera(np.array(FLOOR_CAM["eye"], np.float32), U, V, W)
    r.resize(S, S)
    r.set_environment(raster)
    r.set_subspace()
    assert r.environment()["n_lights"] == 2
    d = pixel_centre_dirs(U, V, W, S, S).reshape(-1, 3)
    t = -FLOOR_CAM["eye"][1] / d[:, 1]
    x = np.asarray(FLOOR_CAM["eye"], np.float64) + t[:, None] * d
    assert (t > 0).all() and (np.abs(x[:, [0, 2]]) < 3.9).all()             # every pixel sees the floor
    wo = -d
    probe = np.random.default_rng(3).choice(len(wo), 64, replace=False)
    k, prev = 2, _sky_radiance(ob, raster, wo[probe], 2)
    while True:
        nxt = _sky_radiance(ob, raster, wo[probe], 2 * k)
        change = (np.abs(nxt - prev).max(1) / nxt.max(1)).max()
        print(f"quadrature: {k} x {k} -> {2 * k} x {2 * k} sub-cells per texel changes the radiance by at most {change:.3g}")
        if change < 1e-5:
            break
        k, prev = 2 * k, nxt
        assert k <= 8
    px = (probe % S)[:, None, None] + (np.arange(4)[None, :, None] + 0.5) / 4 + np.zeros((1, 1, 4))
    py = (probe // S)[:, None, None] + (np.arange(4)[None, None, :] + 0.5) / 4 + np.zeros((1, 4, 1))
    dd = (2 * px / S - 1)[..., None] * np.asarray(U, np.float64) + (2 * py / S - 1)[..., None] * np.asarray(V, np.float64) + np.asarray(W, np.float64)
    dd /= np.linalg.norm(dd, axis=-1, keepdims=True)
    sub = _sky_radiance(ob, raster, -dd.reshape(-1, 3), k).reshape(len(probe), 16, 3).mean(1)
    curve = (np.abs(sub - prev).max(1) / prev.max(1)).max()
    print(f"mean over 4 x 4 positions of a pixel against its centre: at most {curve:.3g}")
    assert curve <= 1e-6
    ref = _lum(_sky_radiance(ob, raster, wo, k)).reshape(S, S)
    ref_flipped = float(_lum(_sky_radiance(ob, raster[::-1].copy(), wo[::16], k)).mean() / ref.reshape(-1)[::16].mean() * ref.mean())
    ref_b, ref_m = ref.reshape(S // 8, 8, S // 8, 8).mean((1, 3)), float(ref.mean())
    # frames: the film keeps the running mean, so frame f's own samples are (f + 1) acc_f - f acc_(f - 1)
    r.clear_accum()
    prev_acc, blocks, means, n = np.zeros((S, S)), [], [], 0
    while True:
        for f in range(n, n + 128):
            r.launch("pt", f)
            r.sync()
            acc = _lum(r.read_accum().astype(np.float64))
            img = (f + 1) * acc - f * prev_acc
            prev_acc = acc
            blocks.append(img.reshape(S // 8, 8, S // 8, 8).mean((1, 3)))
            means.append(img.mean())
        n += 128
        m = np.array(means)
        mean, se = m.mean(), m.std(ddof=1) / math.sqrt(n)
        if se <= 0.005 / 3 * ref_m or n >= 2048:
            break
    assert np.isfinite(prev_acc).all()
    bl = np.array(blocks)
    mean_b, s_b = bl.mean(0), bl.std(0, ddof=1) / math.sqrt(n)
    ok = np.abs(mean_b - ref_b) <= 4 * s_b + 0.005 * ref_b
    z = (mean_b - ref_b) / s_b
    print(f"pt, {n} frames: image mean {mean:.6f} vs quadrature {ref_m:.6f} (ratio {mean / ref_m:.5f}, standard error {se / ref_m:.2e} of it; against the "
          f"flipped raster's {ref_flipped:.6f}: ratio {mean / ref_flipped:.5f}); blocks inside the bar {ok.mean():.4f}, block z-scores mean {z.mean():+.2f} "
          f"rms {np.sqrt((z * z).mean()):.2f} max |z| {np.abs(z).max():.2f}")
    assert se <= 0.005 / 3 * ref_m, (se, ref_m)
    assert ok.mean() >= 0.99, (ok.mean(), np.abs(z).max())
    assert abs(mean / ref_m - 1) <= 0.005
    assert abs(mean / ref_flipped - 1) > 0.005 + 4 * se / ref_flipped


# ---------------------------------------------------------------------------------------------------------------- 9
@pytest.mark.parametrize("name", MAPS)
def test_directly_seen_sky_is_the_map(worlds, pkg, name):
    """The camera above the walls looking straight up, "pt" at subframe 0 (rays through the pixel centres), 33 x 33 so that the
    centre pixel looks exactly along +y: every pixel shows the float64 colour of its float64 primary direction under the bar of
    test_env_color (b).  Measured on the MI355X: 0.15 / 0.11 of the bar at most."""
    from tests.denoise_ref import pixel_centre_dirs
    t = worlds[name]
    r = t["r"]
    S = 33
    try:
        r.set_camera_lookat(UP_CAM["eye"], UP_CAM["lookat"], UP_CAM["up"], UP_CAM["fov"], 1.0)
        r.resize(S, S)
        r.clear_accum()
        r.launch("pt", 0)
        r.sync()
        img = r.read_accum()[..., :3].astype(np.float64).reshape(-1, 3)
    finally:
        r.set_camera_lookat(CAM["eye"], CAM["lookat"], CAM["up"], CAM["fov"], 1.0)
        r.resize(64, 64)
    U, V, W = pkg.camera_frame(UP_CAM["eye"], UP_CAM["lookat"], UP_CAM["up"], UP_CAM["fov"], 1.0)
    d = pixel_centre_dirs(U, V, W, S, S).reshape(-1, 3)
    assert d[(S // 2) * S + S // 2, 1] == 1.0
    assert np.isfinite(img).all()
    u, v = env_ref.dir2uv(d)
    contrast, big = env_ref.local_contrast(t["tex64"], u, v)
    err = np.abs(img - env_ref.env_color(t["raster"], d)).max(-1)
    bar = UV_BOUND * contrast + 1e-6 * big
    _q(f"{name}: directly seen sky against float64, share of the bar", err / bar)
    assert (err <= bar).all()


# ---------------------------------------------------------------------------------------------------------------- F
def test_a_map_too_large_for_the_float_table_is_refused(gpu, pkg):
    """sky_texture(4096, 2048): 1.4 % of the texels of the float CMF do not exceed their predecessor (tests/test_env_table_cpu.py), so
    spcbpt_set_environment refuses the map and names the first; the context renders on, and takes a map that fits.  (On the MI355X
    machine: 0.2 s to make the raster, 0.4 s for the refused call.)"""
    scene = pkg.scenes.cornell_box()
    r = pkg.Renderer(scene, 0)
    cam = scene.camera
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], 1.0)
    r.resize(32, 32)
    t0 = time.time()
    big = pkg.scenes.sky_texture(4096, 2048)
    t1 = time.time()
    with pytest.raises(pkg.SpcbptError, match="too large for the float sampling table") as e:
        r.set_environment(big)
    print(f"sky_texture {t1 - t0:.2f} s, set_environment {time.time() - t1:.2f} s: {e.value}")
    m = re.search(r"texel (\d+) \(column (\d+), row (\d+)\)", str(e.value))
    assert m and 0 < int(m.group(1)) < 4096 * 2048 and int(m.group(1)) == int(m.group(2)) + 4096 * int(m.group(3)), str(e.value)
    assert r.environment()["n_lights"] == 1
    r.set_subspace()
    r.render_frame("SPCBPT_eye", 0)
    r.sync()
    a = r.read_accum()[..., :3]
    assert np.isfinite(a).all() and a.mean() > 0
    r.set_environment(pkg.scenes.sky_texture(16, 8))
    assert r.environment()["n_lights"] == 2
