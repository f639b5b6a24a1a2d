"""The a-trous denoiser on the device (spcbpt_denoise): against the float64 numpy recomputation of the formula (tests/denoise_ref.py)
and against spcbpt_denoise_host, both run on the device's own read-back buffers, under the host test's bar (1e-4 of the largest
channel: tests/test_denoise_host.py derives it; the library under test is the IEEE build); and what the feature is for -- a 4-frame
image closer to a disjoint 512-frame mean after denoising than before.

Measured on the MI355X: see DESIGN.md 8c."""
import os
import subprocess

import numpy as np
import pytest

from tests.denoise_ref import atrous_ref, tone_map_codes
from tests.test_gpu_features import _camera, _rays
from tests.test_gpu_mesh_light import _renderer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-4
STATE, INVALID = -5, -1
FRAMES, REF_FRAMES = 4, 512


def _rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - b) ** 2)))


def _noisy_and_reference(r, alg, frames=FRAMES, ref_frames=REF_FRAMES, denoise=None):
    """`frames` subframes of `alg` with a feature launch beside each, then -- if asked -- ref_frames more "pt" subframes on the same film:
    the reference is the mean of the LATER subframes alone, (n A_n - 4 A_4) / (n - 4), so it shares no sample with the 4-frame image."""
    for f in range(frames):
        if alg == "pt":
            r.launch("pt", f)
        else:
            r.render_frame(alg, f)
        r.launch_features(f)
    out = dict(accum=r.read_accum().copy(), frame=r.read_frame().copy())
    out["albedo"], out["normal_depth"] = (a.copy() for a in r.read_features())
    if denoise is not None:
        r.denoise(**denoise)
        out["denoised"], out["denoised8"] = (a.copy() for a in r.read_denoised())
    if ref_frames:
        n = frames + ref_frames
        for f in range(frames, n):
            r.launch("pt", f)
        total = r.read_accum()[..., :3].astype(np.float64)
        out["reference"] = (n * total - frames * out["accum"][..., :3].astype(np.float64)) / ref_frames
    return out


# ------------------------------------------------------------------------------------------------------------ the filter itself
@pytest.fixture(scope="module", params=[(48, 32), (43, 29)], ids=["48x32", "43x29"])
def box(request, gpu, pkg, hip_lib):
    assert hip_lib.spcbpt_build_arithmetic().decode() == "ieee"
    w, h = request.param
    scene = pkg.scenes.cornell_box()
    r = _renderer(pkg, scene, w, h)
    d = _noisy_and_reference(r, "pt", ref_frames=0)
    d.update(r=r, w=w, h=h, cam=_camera(pkg, scene, w, h))
    return d


@pytest.mark.parametrize("iterations", [1, 5])
def test_device_filter_matches_formula_and_host(pkg, box, iterations):
    r, (eye, U, V, W) = box["r"], box["cam"]
    sigma = (2.0, 0.5, 0.2)
    r.denoise(iterations, *sigma)
    den, den8 = r.read_denoised()
    assert np.isfinite(den).all() and (den[..., 3] == 1).all()
    ref = atrous_ref(box["accum"], box["albedo"], box["normal_depth"], U, V, W, iterations, *sigma)
    host = pkg.api.denoise_host(box["accum"], box["albedo"], box["normal_depth"], eye, U, V, W, iterations, *sigma)
    top = ref.max()
    d_ref, d_host = np.abs(den[..., :3] - ref).max() / top, np.abs(den[..., :3].astype(np.float64) - host[..., :3]).max() / top
    print(f"{box['w']}x{box['h']}, {iterations} iterations: device - float64 {d_ref:.3g}, device - host {d_host:.3g} (of the largest channel {top:.3g})")
    assert d_ref <= BAR and d_host <= BAR
    assert np.abs(den[..., :3] - box["accum"][..., :3]).max() > 1e-3         # it filtered
    # accum and frame are bit for bit what they were
    assert r.read_accum().tobytes() == box["accum"].tobytes() and r.read_frame().tobytes() == box["frame"].tobytes()
    # the RGBA8 output is the film's tone map of the float output: +-1 code where the float64 value sits at a quantisation tie
    codes = tone_map_codes(den[..., :3])
    want = np.minimum(np.floor(codes), 255)
    diff = den8[..., :3].astype(np.int64) - want
    tie = np.abs(codes - np.round(codes)) < 1e-3
    assert (den8[..., 3] == 255).all()
    assert (diff[~tie] == 0).all() and (np.abs(diff) <= 1).all(), (np.abs(diff).max(), int((diff != 0).sum()))


def test_errors(gpu, pkg):
    scene = pkg.scenes.cornell_box()
    w, h = 48, 32

    def fails(fn, code, text=None):
        with pytest.raises(pkg.SpcbptError) as e:
            fn()
        assert f"({code})" in str(e.value), str(e.value)
        if text:
            assert text in str(e.value), str(e.value)

    r = _renderer(pkg, scene, w, h)
    r.launch("pt", 0)
    fails(lambda: r.denoise(), STATE, "feature")              # before any feature launch
    fails(lambda: r.read_denoised(), STATE)
    r.launch_features(0)
    for it in (0, 9, -1):
        fails(lambda: r.denoise(it), INVALID, "iterations")
    r.launch_deferred("pt", 1)
    fails(lambda: r.denoise(), STATE, "deferred")
    r.merge_deferred(True)
    r.denoise()
    a, _ = r.read_denoised()
    assert np.isfinite(a).all() and a[..., :3].mean() > 0
    r.resize(w, h)
    fails(lambda: r.denoise(), STATE, "feature")              # a resize forgets the features ...
    fails(lambda: r.read_denoised(), STATE)                   # ... and the result
    r.launch("pt", 0)
    r.launch("pt", 1)
    r.launch_features(0)
    r.denoise()
    b, _ = r.read_denoised()
    assert np.array_equal(a, b)                               # the same film and features give the same image


# ------------------------------------------------------------------------------------------------------------ what it is for
@pytest.fixture(scope="module")
def box64(gpu, pkg):
    """Cornell box at 64 x 64: the 4-frame "pt" film, its denoised image (default parameters) and the disjoint 512-frame "pt" mean."""
    scene = pkg.scenes.cornell_box()
    r = _renderer(pkg, scene, 64, 64, tuple_="minimal")
    d = _noisy_and_reference(r, "pt", denoise=dict(iterations=5))
    d.update(r=r, scene=scene)
    return d


def test_denoised_pt_is_closer_to_the_reference(box64):
    noisy, den = _rmse(box64["accum"][..., :3], box64["reference"]), _rmse(box64["denoised"][..., :3], box64["reference"])
    print(f"cornell 64x64, 4 frames of pt: RMSE {noisy:.4f} -> {den:.4f} denoised (ratio {den / noisy:.3f})")
    assert den < noisy


def test_denoised_spcbpt_eye_is_closer_to_the_reference(box64):
    r = box64["r"]
    r.resize(64, 64)
    d = _noisy_and_reference(r, "SPCBPT_eye", ref_frames=0, denoise=dict(iterations=5))
    noisy, den = _rmse(d["accum"][..., :3], box64["reference"]), _rmse(d["denoised"][..., :3], box64["reference"])
    print(f"cornell 64x64, 4 frames of SPCBPT_eye (minimal tuple): RMSE {noisy:.4f} -> {den:.4f} denoised (ratio {den / noisy:.3f})")
    assert den < noisy


def test_textured_floor_keeps_its_checker(gpu, pkg):
    """The bedroom's floor carries a checker texture: over the floor's pixels the denoised image is closer to the 512-frame mean (mean
    absolute difference) than the 4-frame film -- a filter that blurred the albedo would lose here, the checker's contrast is 15:1."""
    scene = pkg.scenes.bedroom(target_tris=20_000, tex_size=64)
    w = h = 64
    r = _renderer(pkg, scene, w, h)
    d = _noisy_and_reference(r, "pt", denoise=dict(iterations=5))
    _, tri, _ = r.trace_closest(_rays(*_camera(pkg, scene, w, h), w, h)[0])
    tri = tri.reshape(h, w)
    nt = len(scene.indices)
    floor = (tri >= 0) & (tri < nt) & (np.asarray(scene.tri_material)[np.clip(tri, 0, nt - 1)] == 0)
    assert scene.materials[0].get("albedo_tex", 0) > 0 and floor.sum() > 200
    ref = d["reference"]
    mad = lambda a: float(np.abs(a[..., :3].astype(np.float64) - ref)[floor].mean())
    noisy, den = mad(d["accum"]), mad(d["denoised"])
    whole = _rmse(d["denoised"][..., :3], ref) / _rmse(d["accum"][..., :3], ref)
    contrast = d["albedo"][..., 0][floor]
    print(f"bedroom 64x64, {int(floor.sum())} floor pixels (albedo {contrast.min():.3f} .. {contrast.max():.3f}): mean |error| {noisy:.4f} -> {den:.4f} "
          f"denoised (ratio {den / noisy:.3f}); whole-image RMSE ratio {whole:.3f}")
    assert den < noisy


def test_render_tool_denoises(box64, pkg, tmp_path):
    """tools/spcbpt_render --denoise --features on the Cornell box's .scene file: the five extra files, and a denoised PFM closer to the
    reference than the tool's own 4-frame PFM."""
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "spcbpt_render"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    path = pkg.scenes.write_scene(box64["scene"], str(tmp_path), "cornell")
    out = os.path.join(str(tmp_path), "tool")
    cmd = [os.path.join(ROOT, "tools", "spcbpt_render"), path, str(tmp_path), "--alg", "pt", "--dim=64x64", "--frames", str(FRAMES), "--denoise", "--features", "--out", out]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:]

    def pfm(name):
        raw = open(out + name, "rb").read()
        head = raw.split(b"\n", 3)
        assert head[0] == b"PF" and head[1] == b"64 64", head[:2]
        return np.frombuffer(head[3], np.float32).reshape(64, 64, 3)

    film, den, albedo, normal, depth = (pfm(n) for n in (".pfm", "_denoised.pfm", "_albedo.pfm", "_normal.pfm", "_depth.pfm"))
    ppm = open(out + "_denoised.ppm", "rb").read()
    assert ppm.startswith(b"P6\n64 64\n255\n") and len(ppm) == len(b"P6\n64 64\n255\n") + 64 * 64 * 3
    for a in (film, den, albedo, normal, depth):
        assert np.isfinite(a).all()
    assert np.allclose(albedo, box64["albedo"][..., :3], atol=1e-6) and np.allclose(depth[..., 0], box64["normal_depth"][..., 3], rtol=1e-5)
    assert np.allclose(normal, box64["normal_depth"][..., :3], atol=1e-6)
    noisy, clean = _rmse(film, box64["reference"]), _rmse(den, box64["reference"])
    print(f"tool: RMSE {noisy:.4f} -> {clean:.4f} denoised")
    assert clean < noisy
