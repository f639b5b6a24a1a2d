"""The device's Disney BSDF (csrc/dev_bsdf.h, through SPCBPT_UNIT_BSDF) against the float64 definition of tests/bsdf_ref.py: its sampled
directions are distributed as the definition's Pdf says, and Sample / Eval / Pdf agree with the definition record by record on the
families of tests/test_bsdf_definition_cpu.py, inside the bound whose constants that file measured from the FP32 ORACLE -- the device
is held to what FP32 arithmetic of these formulas was seen to deliver on the CPU, never to itself.  One image closes the loop: a floor
with every lobe but the clearcoat switched on, rendered and compared with a float64 quadrature of the direct light that takes its f
from the definition.  Bars and conventions are those of the CPU file's docstring."""
import math

import numpy as np
import pytest

from tests import bsdf_ref as B
from tests import test_bsdf_definition_cpu as D
from tests.test_gpu_mesh_light import _frames, _light_geometry, _lum, _quadrature_nodes, _renderer
from tests.test_gpu_units import OP

pytestmark = pytest.mark.gpu
CHUNK = 500_000          # records per launch: 48 MB in, 24 MB out


@pytest.fixture(scope="module")
def unit(gpu, pkg):
    r = pkg.Renderer(pkg.scenes.cornell_box(), 0)       # the BSDF op needs neither a tuple nor a sampler

    def run(words):
        """direction, seed afterwards, Eval, Pdf of every record"""
        out = np.concatenate([r.unit(OP["BSDF"], words[s:s + CHUNK], 12) for s in range(0, len(words), CHUNK)])
        g = out.view(np.float32)
        return g[:, 0:3], out[:, 3], g[:, 4:7], g[:, 7]
    return run


# ------------------------------------------------------------------------------------------------------ sampling density
@pytest.mark.parametrize("k", range(len(D.CONFIGS)))
def test_device_samples_are_distributed_as_pdf(unit, k):
    """The chi^2 of the CPU file on the device's own sampled directions: 1 000 000 seeds, 12 x 24 cells and the below-surface bin,
    tail probability above 1e-6; and the below-surface count against the definition's mass at 5 sigma of the binomial."""
    cfg = D.CONFIGS[k]
    cells, change, s = D.expected_cells(B.pdf, cfg["mat"], cfg["N"], cfg["V"])
    assert change <= 1e-3
    seeds, _ = D.draw_uniforms(k)
    counts = np.zeros(D.NC * D.NPHI + 1, np.int64)
    for a in range(0, len(seeds), CHUNK):
        n = len(seeds[a:a + CHUNK])
        words = D.records(cfg["mat"], np.tile(cfg["N"], (n, 1)), np.tile(cfg["V"], (n, 1)), np.tile(cfg["N"], (n, 1)), seeds[a:a + CHUNK])
        direction, after, _, _ = unit(words)
        assert np.array_equal(after, B.draws(seeds[a:a + CHUNK])[3])
        assert np.isfinite(direction).all()
        counts += D.bin_directions(cfg["N"], direction.astype(np.float64))
    x, df, p = D.chi2_of(counts, cells)
    n, mass = int(counts.sum()), 1.0 - float(cells.sum())
    below, sigma = counts[-1] / n, math.sqrt(mass * (1.0 - mass) / n)
    print(f"device: {cfg['name']}: chi^2 = {x:.1f} with {df} degrees of freedom, tail probability {p:.3g}; below the surface {below:.5f} "
          f"against {mass:.5f} ({(below - mass) / sigma:+.2f} sigma)")
    assert p > 1e-6, (x, df)
    assert abs(below - mass) <= 5.0 * sigma


# ------------------------------------------------------------------------------------------------------ pointwise
def test_device_against_the_definition(unit):
    """Every family of the CPU file, every record (judge: finite, the integer LCG's seed, Eval exactly zero where N.L or N.V is exactly
    <= 0, the pinned seeds on the definition's branch), inside the bound with the constants measured from the oracle, and within
    1e-5 where t2 >= 0.05 without clearcoat."""
    samples, failures = D.judge("device", unit)
    c0, c2, c1 = D.fit_constants(samples)
    print(f"device: the same fit on the device's errors would give C0 = {c0:.3g}, C2 = {c2:.3g}, C1 = {c1:.3g}; held to the oracle's {D.C0:g}, {D.C2:g}, {D.C1:g}")
    assert not failures, failures


def test_device_pdf_of_the_opposite_direction_is_not_a_number(unit):
    """L = -V is 0 / 0 in the formula: the device answers as the oracle and the definition do (tests/test_bsdf_definition_cpu.py)."""
    _, _, f, pdf = unit(D.antipodal())
    assert not np.isfinite(pdf).any() and (f == 0).all()


def test_device_eval_is_reciprocal(unit):
    """Eval with V and L swapped agrees with itself inside the same bound (the definition is reciprocal to 1e-13)."""
    fams = D.families()
    for name in ("random", "peak", "grazing", "retro", "black / saturated", "ratio edges"):
        words = fams[name]
        swapped = words.copy()
        swapped[:, 15:18], swapped[:, 18:21] = words[:, 18:21], words[:, 15:18]
        d = D.definition(words)
        a, b = unit(words)[2].astype(np.float64), unit(swapped)[2].astype(np.float64)
        keep = D.random_mask(d) if name == "random" else np.ones(len(words), bool)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.where(d["f_scale"] > 0, np.abs(a - b).max(-1) / (d["f_scale"] * D.EPS32), np.where((a == b).all(-1), 0.0, np.inf))[keep]
        bound = D.bound(d, 1)[keep]
        print(f"device: reciprocity, {name:20s} n = {len(e):6d}  |f(V, L) - f(L, V)| / (2^-24 scale) 50 / 99 / 100 % = "
              + " / ".join(f"{q:.3g}" for q in np.quantile(e, [0.5, 0.99, 1.0])) + f"; worst against the bound {float((e / bound).max()):.3f}")
        assert (e <= bound).all(), (name, float((e / bound).max()))


# ------------------------------------------------------------------------------------------------------ one image
FLOOR = dict(color=(0.7, 0.65, 0.6), metallic=0.3, roughness=0.5, specular=0.5, specular_tint=0.5, subsurface=0.3, sheen=0.5, sheen_tint=0.5, clearcoat=0.0)
W = H = 32
FRAMES = dict(pt=1024, SPCBPT_eye=64)      # measured standard error of the image mean / reference: pt 1.87e-3 at 512, 1.31e-3 at 1024; SPCBPT_eye 2.27e-3 at 32, 1.60e-3 at 64


def _direct_light64(mat, Le, P, x, wo, level, chunk=512):
    """Float64 direct radiance (m, 3) leaving floor points x (normal +y) towards wo from the front sides of the lamp's faces P, f from
    the definition (tests/test_gpu_mesh_light.py: _direct_light takes it from the oracle)."""
    nodes, wts, nrm = _quadrature_nodes(P, level)
    out = np.zeros((len(x), 3))
    N = np.array([0.0, 1.0, 0.0])
    for s in range(0, len(x), chunk):
        d = nodes[None, :, :] - x[s:s + chunk, None, :]
        r2 = (d * d).sum(-1)
        wi = d / np.sqrt(r2)[..., None]
        cos_s, cos_l = wi[..., 1], -(wi * nrm[None, :, :]).sum(-1)
        g = np.where((cos_s > 0) & (cos_l > 0), cos_s * cos_l / r2, 0.0) * wts[None, :]
        f = B.eval(mat, N, wo[s:s + chunk, None, :], wi)
        out[s:s + chunk] = (f * g[..., None]).sum(1) * np.asarray(Le, np.float64)[None, :]
    return out


@pytest.fixture(scope="module")
def floor_truth(gpu, pkg):
    """The lamp over a floor with every lobe but the clearcoat on (with it, the inherited Pdf makes "pt" biased by the gap the CPU file
    pins), and the float64 expectation of every pixel: the jittered camera draws uniformly inside a pixel, so a pixel's expectation is
    the mean of the direct light over its footprint -- the two-point Gauss rule in k x k cells per pixel, k doubled until no block
    moves by 1e-5."""
    scene = pkg.scenes.lamp_floor()
    scene.materials[0] = dict(FLOOR)
    r = _renderer(pkg, scene, W, H, light=(20000, 16, 1), tuple_="trained")
    cam = scene.camera
    eye = np.array(cam["eye"], np.float64)
    U, V, Wv = (np.asarray(a, np.float64) for a in pkg.camera_frame(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H))
    P64, _, _ = _light_geometry(pkg, scene)
    Le = scene.mesh_lights[0]["emission"]

    def image(k, level):
        cell, g = np.arange(W * k) + 0.5, 0.5 / math.sqrt(3.0)
        sub = np.stack([cell - g, cell + g], 1).ravel() / k               # the two Gauss points of each of the k cells per pixel side
        px, py = np.meshgrid(sub, sub)
        d = (2 * px / W - 1)[..., None] * U + (2 * py / H - 1)[..., None] * V + Wv
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        t = -eye[1] / d[..., 1]
        assert (t > 0).all()
        x = eye + t[..., None] * d
        assert (np.abs(x[..., [0, 2]]) < 4).all()                          # every pixel sees the floor, nothing else
        rad = _direct_light64(FLOOR, Le, P64, x.reshape(-1, 3), -d.reshape(-1, 3), level)
        return rad.reshape(H, 2 * k, W, 2 * k, 3).mean((1, 3))

    level, prev = 1, image(1, 1)
    while True:                                                            # the lamp's subdivision, at pixel centres
        nxt = image(1, level + 1)
        change = float((np.abs(nxt - prev).max(-1) / nxt.max(-1)).max())
        print(f"quadrature: level {level} -> {level + 1} changes the direct light by at most {change:.3g}")
        level, prev = level + 1, nxt
        if change < 1e-5:
            break
        assert level < 5
    k = 1
    while True:                                                            # the pixel footprint
        nxt = image(2 * k, level)
        blocks = lambda a: a.reshape(H // 8, 8, W // 8, 8, 3).mean((1, 3))
        change = float((np.abs(blocks(nxt) - blocks(prev)).max(-1) / blocks(nxt).max(-1)).max())
        print(f"quadrature: {k} -> {2 * k} Gauss cells per pixel side change the block means by at most {change:.3g}")
        k, prev = 2 * k, nxt
        if change < 1e-5:
            break
        assert k < 8
    return dict(r=r, ref_blocks=prev.reshape(H // 8, 8, W // 8, 8, 3).mean((1, 3)), ref_mean=prev.mean((0, 1)))


@pytest.mark.parametrize("alg", ["pt", "SPCBPT_eye"])
def test_an_all_lobes_floor_against_the_definitions_quadrature(floor_truth, alg):
    """The bars of tests/test_gpu_mesh_light.py::test_direct_light_against_quadrature at 32 x 32: every 8 x 8 block within 4 s + 0.005 ref,
    the image mean within 0.5 %, with the smallest power of two of frames at which the mean's standard error is below 0.005 / 3 of the
    reference (FRAMES; measured on the MI355X, the standard errors are beside the assertion)."""
    t = floor_truth
    n = FRAMES[alg]
    acc, blocks, means = _frames(t["r"], alg, n, W, H)
    assert np.isfinite(acc).all()
    ref_b, ref_m = _lum(t["ref_blocks"]), float(_lum(t["ref_mean"]))
    b = _lum(blocks)
    mean_b, s_b = b.mean(0), b.std(0, ddof=1) / math.sqrt(n)
    ok = np.abs(mean_b - ref_b) <= 4 * s_b + 0.005 * ref_b
    m = _lum(means)
    mean, se = m.mean(), m.std(ddof=1) / math.sqrt(n)
    z = (mean_b - ref_b) / s_b
    print(f"{alg}: {n} frames: image mean {mean:.6f} vs quadrature {ref_m:.6f} (ratio {mean / ref_m:.5f}, standard error {se / ref_m:.2e} of it); "
          f"blocks inside the bar {ok.mean():.4f}, max |z| {np.abs(z).max():.2f}")
    assert se <= 0.005 / 3 * ref_m, (se, ref_m)          # 1.667e-3 of the reference; measured on the MI355X: FRAMES
    assert ok.all(), (ok.mean(), np.abs(z).max())
    assert abs(mean / ref_m - 1) <= 0.005
