"""The film's second moment on the device (spcbpt_set_film_moments), the film error (spcbpt_film_error) and the variance-guided
a-trous denoiser (spcbpt_denoise_variance): against float64 recomputations from the device's own read-backs (tests/denoise_var_ref.py)
and against the host forms, under the bars tests/test_film_moments_host.py derives (update 1e-4 n max x^2, error 1e-5 relative, filter
1e-4 of the largest channel; the library under test is the IEEE build); that a context which does not ask keeps its film bits; and
what the feature is for -- a filter that still helps at 64 frames, and a renderer that can say when to stop.

Measured on the MI355X: see DESIGN.md 8e."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.denoise_ref import tone_map_codes
from tests.denoise_var_ref import atrous_var_ref, film_error_ref
from tests.test_gpu_features import _camera
from tests.test_gpu_mesh_light import _renderer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-4
STATE = -5
FRAMES = 8


def _rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - b) ** 2)))


def _fails(pkg, fn, code, text=None):
    with pytest.raises(pkg.SpcbptError) as e:
        fn()
    assert f"({code})" in str(e.value), str(e.value)
    if text:
        assert text in str(e.value), str(e.value)


def _m2_from_films(films):
    """M2 in float64 from the film after every merge, A_0 .. A_{n-1}: the samples x_f = (f + 1) A_f - f A_{f-1}, then
    sum_f (x_f - A_{f-1}) (x_f - A_f).  Returns (M2, max_f x_f^2)."""
    A = [a[..., :3].astype(np.float64) for a in films]
    m2, top = np.zeros_like(A[0]), A[0] ** 2
    for f in range(1, len(A)):
        x = (f + 1) * A[f] - f * A[f - 1]
        m2 += (x - A[f - 1]) * (x - A[f])
        top = np.maximum(top, x ** 2)
    return m2, top


# ------------------------------------------------------------------------------------------------------------ moments on the device
@pytest.fixture(scope="module", params=[(48, 32), (43, 29)], ids=["48x32", "43x29"])
def box(request, gpu, pkg, hip_lib):
    """The Cornell box, 8 subframes of "pt" with the moments on and a feature launch beside each: the film after every merge, the plane,
    the features -- and the same launches on a second context with the moments off."""
    assert hip_lib.spcbpt_build_arithmetic().decode() == "ieee"
    w, h = request.param
    scene = pkg.scenes.cornell_box()
    r = _renderer(pkg, scene, w, h)
    assert r.film_moments() is False
    r.set_film_moments(True)
    assert r.film_moments() is True
    off = _renderer(pkg, scene, w, h)
    films = []
    for f in range(FRAMES):
        r.launch("pt", f)
        r.launch_features(f)
        off.launch("pt", f)
        films.append(r.read_accum().copy())
    d = dict(r=r, off=off, w=w, h=h, scene=scene, films=films, accum=films[-1], frame=r.read_frame().copy(), m2n=r.read_film_moments().copy(),
             cam=_camera(pkg, scene, w, h))
    d["albedo"], d["normal_depth"] = (a.copy() for a in r.read_features())
    return d


def test_device_moments_match_float64(box):
    m2n = box["m2n"]
    assert np.all(m2n[..., 3] == FRAMES)
    m2, top = _m2_from_films(box["films"])
    dev = np.abs(m2n[..., :3] - m2)
    unit = FRAMES * top
    print(f"{box['w']}x{box['h']}: largest |M2 - float64| {dev.max():.3e}; {(dev[unit > 0] / unit[unit > 0]).max():.3e} of n max x^2 (bar 1e-4)")
    assert np.all(dev <= 1e-4 * unit)
    assert m2n[..., :3].max() > 1e-3


def test_film_bits_do_not_depend_on_the_switch(pkg, box):
    off = box["off"]
    assert off.read_accum().tobytes() == box["accum"].tobytes() and off.read_frame().tobytes() == box["frame"].tobytes()
    for fn in (off.read_film_moments, off.film_error, off.denoise_variance):
        _fails(pkg, fn, STATE, "moments")


def test_film_error_matches_float64_and_repeats(pkg, box):
    r = box["r"]
    a, b = r.film_error(), r.film_error()
    assert a == b                                                        # no atomics: the same film, the same bits
    pixels, mean, top = film_error_ref(box["accum"], box["m2n"])
    host = pkg.api.film_error_host(box["accum"], box["m2n"])
    print(f"{box['w']}x{box['h']}: film error mean {a['mean']:.6g} (float64 {mean:.6g}), max {a['max']:.6g} (float64 {top:.6g})")
    assert a["pixels"] == pixels == host["pixels"] == box["w"] * box["h"]
    assert abs(a["mean"] / mean - 1) <= 1e-5 and abs(a["max"] / top - 1) <= 1e-5
    assert abs(a["mean"] / host["mean"] - 1) <= 1e-5 and abs(a["max"] / host["max"] - 1) <= 1e-5


@pytest.mark.parametrize("iterations", [1, 5])
def test_device_filter_matches_formula_and_host(pkg, box, iterations):
    r, (eye, U, V, W) = box["r"], box["cam"]
    sigma = (4.0, 0.5, 0.2)
    r.denoise_variance(iterations, *sigma)
    den, den8 = r.read_denoised()
    assert np.isfinite(den).all() and (den[..., 3] == 1).all()
    args = (box["accum"], box["m2n"], box["albedo"], box["normal_depth"])
    ref = atrous_var_ref(*args, U, V, W, iterations, *sigma)
    host = pkg.api.denoise_variance_host(*args, eye, U, V, W, iterations, *sigma)
    top = ref.max()
    d_ref, d_host = np.abs(den[..., :3] - ref).max() / top, np.abs(den[..., :3].astype(np.float64) - host[..., :3]).max() / top
    print(f"{box['w']}x{box['h']}, {iterations} iterations: device - float64 {d_ref:.3g}, device - host {d_host:.3g} (of the largest channel {top:.3g})")
    assert d_ref <= BAR and d_host <= BAR
    assert np.abs(den[..., :3] - box["accum"][..., :3]).max() > 1e-3         # it filtered
    # accum, frame, the features and the moments are bit for bit what they were
    assert r.read_accum().tobytes() == box["accum"].tobytes() and r.read_frame().tobytes() == box["frame"].tobytes()
    alb, nd = r.read_features()
    assert alb.tobytes() == box["albedo"].tobytes() and nd.tobytes() == box["normal_depth"].tobytes()
    assert r.read_film_moments().tobytes() == box["m2n"].tobytes()
    # the RGBA8 output is the film's tone map of the float output: +-1 code where the float64 value sits at a quantisation tie
    codes = tone_map_codes(den[..., :3])
    want = np.minimum(np.floor(codes), 255)
    diff = den8[..., :3].astype(np.int64) - want
    tie = np.abs(codes - np.round(codes)) < 1e-3
    assert (den8[..., 3] == 255).all()
    assert (diff[~tie] == 0).all() and (np.abs(diff) <= 1).all(), (np.abs(diff).max(), int((diff != 0).sum()))


# ------------------------------------------------------------------------------------------------------------ which launches count
def test_bands_restart_deferred_clear_and_resize(gpu, pkg):
    scene = pkg.scenes.cornell_box()
    w, h = 43, 29
    r = _renderer(pkg, scene, w, h, tuple_="minimal")
    r.set_film_moments(True)
    assert not r.read_film_moments().any()                     # before the first merge: zeros
    assert r.film_error() == {"pixels": 0, "mean": 0.0, "max": 0.0}
    n = lambda: r.read_film_moments()[..., 3]
    r.launch("pt", 0)
    assert np.all(n() == 1) and r.film_error()["pixels"] == 0  # one frame: no pixel has two samples
    r.launch("pt", 1)
    assert np.all(n() == 2) and r.film_error()["pixels"] == w * h
    # a banded launch raises n on its rows only: bands 1 and 3 of rows (8, h, 2)
    r.launch("pt", 2, (8, h, 2))
    rows = np.zeros(h, bool)
    rows[8:16] = True
    rows[24:h] = True
    assert np.all(n()[rows] == 3) and np.all(n()[~rows] == 2)
    # a deferred frame counts when it is kept and not when it is dropped
    before = r.read_film_moments().copy()
    r.launch_deferred("pt", 3)
    r.merge_deferred(False)
    assert r.read_film_moments().tobytes() == before.tobytes()
    r.launch_deferred("pt", 3)
    r.merge_deferred(True)
    assert np.all(n() == before[..., 3] + 1)
    # "SPCBPT_eye" and "lt" end in the same merge
    r.render_frame("SPCBPT_eye", 4)
    r.render_frame("lt", 5)
    assert np.all(n() == before[..., 3] + 3)
    # the batched merge keeps no moments: refused while the switch is on, as before when it is off
    r.launch("light trace", 7)
    r.build_sampler()
    _fails(pkg, lambda: r.launch_eye_batch([6]), STATE, "moments")
    # subframe 0 restarts
    r.launch("pt", 0)
    m = r.read_film_moments()
    assert np.all(m[..., 3] == 1) and not m[..., :3].any()
    r.launch("pt", 1)
    r.clear_accum()
    assert not r.read_film_moments().any()
    r.launch("pt", 0)
    r.resize(w, h)
    assert not r.read_film_moments().any() and r.film_moments()  # a resize forgets the plane, not the switch
    r.launch("pt", 0)
    r.launch("pt", 1)
    assert np.all(n() == 2)
    r.set_film_moments(False)
    _fails(pkg, r.read_film_moments, STATE, "moments")
    r.launch("light trace", 9)
    r.build_sampler()
    r.launch_eye_batch([2])
    r.sync()
    r.set_film_moments(True)                                   # switched on in mid-film: n counts the merges since
    r.launch("pt", 3)
    assert np.all(n() == 1)


def test_preconditions_of_the_filter(gpu, pkg):
    scene = pkg.scenes.cornell_box()
    r = _renderer(pkg, scene, 48, 32)
    r.set_film_moments(True)
    r.launch("pt", 0)
    _fails(pkg, r.denoise_variance, STATE, "feature")
    r.launch_features(0)
    for it in (0, 9):
        _fails(pkg, lambda: r.denoise_variance(it), -1, "iterations")
    r.launch_deferred("pt", 1)
    _fails(pkg, r.denoise_variance, STATE, "deferred")
    r.merge_deferred(True)
    r.denoise_variance()
    a, _ = r.read_denoised()
    assert np.isfinite(a).all() and a[..., :3].mean() > 0
    r.resize(48, 32)
    _fails(pkg, r.denoise_variance, STATE, "feature")


# ------------------------------------------------------------------------------------------------------------ the reduction
def test_film_error_over_several_blocks(gpu, pkg):
    """131 x 67: 8 777 pixels, 35 blocks of the reduction, the last one ragged."""
    scene = pkg.scenes.cornell_box()
    w, h = 131, 67
    r = _renderer(pkg, scene, w, h)
    r.set_film_moments(True)
    for f in range(4):
        r.launch("pt", f)
    a, b = r.film_error(), r.film_error()
    assert a == b
    acc, m2n = r.read_accum(), r.read_film_moments()
    pixels, mean, top = film_error_ref(acc, m2n)
    print(f"{w}x{h}: film error mean {a['mean']:.6g} (float64 {mean:.6g}), max {a['max']:.6g} (float64 {top:.6g}) over {a['pixels']} pixels")
    assert a["pixels"] == pixels == w * h
    assert abs(a["mean"] / mean - 1) <= 1e-5 and abs(a["max"] / top - 1) <= 1e-5


# ------------------------------------------------------------------------------------------------------------ what it is for
def test_guided_filter_helps_at_4_and_at_64_frames(gpu, pkg):
    """Cornell box at 64 x 64, "pt": the variance-guided image is closer to a disjoint 512-frame mean than the film at 4 and at 64
    frames.  The plain filter's RMSE is printed beside it (recorded, not gated)."""
    scene = pkg.scenes.cornell_box()
    r = _renderer(pkg, scene, 64, 64)
    r.set_film_moments(True)
    shots = {}
    for f in range(64):
        r.launch("pt", f)
        r.launch_features(f)
        if f + 1 in (4, 64):
            s = dict(accum=r.read_accum()[..., :3].astype(np.float64), error=r.film_error()["mean"])
            r.denoise_variance(5)
            s["guided"] = r.read_denoised()[0][..., :3].astype(np.float64)
            r.denoise(5)
            s["plain"] = r.read_denoised()[0][..., :3].astype(np.float64)
            shots[f + 1] = s
    for f in range(64, 64 + 512):
        r.launch("pt", f)
    ref = ((64 + 512) * r.read_accum()[..., :3].astype(np.float64) - 64 * shots[64]["accum"]) / 512
    for n, s in shots.items():
        noisy, guided, plain = (_rmse(s[k], ref) for k in ("accum", "guided", "plain"))
        print(f"cornell 64x64, {n} frames of pt (film error {s['error']:.4f}): RMSE {noisy:.4f} -> {guided:.4f} variance-guided, {plain:.4f} plain")
        assert guided < noisy
    assert shots[64]["error"] < shots[4]["error"]


def test_render_tool_stops_at_the_target_error(gpu, pkg, tmp_path):
    """tools/spcbpt_render --target-error on the Cornell box's .scene file stops before --frames, and the error it reports is
    spcbpt_film_error's after that many frames."""
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "spcbpt_render"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    path = pkg.scenes.write_scene(pkg.scenes.cornell_box(), str(tmp_path), "cornell")
    scene, _ = pkg.load_scene_file(path, str(tmp_path))
    cam = scene.camera
    r = pkg.Renderer(scene, 0)
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], 1.0)
    r.resize(64, 64)
    r.set_film_moments(True)
    errors = {}
    for f in range(32):
        r.launch("pt", f)
        if (f + 1) % 4 == 0:
            errors[f + 1] = r.film_error()["mean"]
    target = 0.5 * (errors[12] + errors[16])
    want = min(n for n, e in errors.items() if e <= target)
    out = os.path.join(str(tmp_path), "tool")
    cmd = [os.path.join(ROOT, "tools", "spcbpt_render"), path, str(tmp_path), "--alg", "pt", "--dim=64x64", "--frames", "64", "--target-error", repr(target),
           "--check-every", "4", "--denoise-variance", "--out", out]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:]
    m = re.search(r"(\d+) frames used, error reached ([0-9.eE+-]+)", p.stdout)
    assert m, p.stdout[-3000:]
    used, reached = int(m.group(1)), float(m.group(2))
    print(f"tool: target {target:.6g}: {used} frames used, error reached {reached:.6g}; film_error after {want} frames: {errors[want]:.6g}")
    assert used == want < 64 and reached <= target
    assert abs(reached / errors[used] - 1) <= 1e-5
    for name in (".pfm", "_denoised.pfm", "_denoised.ppm"):
        assert os.path.getsize(out + name) > 64 * 64 * 3
