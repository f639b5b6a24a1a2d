"""History reprojection on the device (spcbpt_history_*): the prior and the resolved image against the float64 restatement of the
formula (tests/reproject_ref.py) and against the host forms, all run on the device's own read-back planes, under the host test's bar
(1e-4 of the largest value: tests/test_reproject_host.py; the library under test is the IEEE build); chaining, the state errors,
what the feature is for -- the first frames after a camera move closer to a converged image than the film -- the viewer's switch in
its three pipeline modes, and tools/spcbpt_viewer --reproject.

Measured on the MI355X: see DESIGN.md 8f."""
import os
import subprocess

import numpy as np
import pytest

from tests import reproject_ref as rr
from tests.denoise_ref import tone_map_codes
from tests.test_gpu_mesh_light import _renderer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-4
STATE, INVALID = -5, -1
SIGMA_N, SIGMA_X_FRACTION, MAX_HISTORY = 0.25, 0.005, 32.0


def _rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64)[..., :3] - np.asarray(b, np.float64)[..., :3]) ** 2)))


def _diag(scene):
    v = np.asarray(scene.vertices, np.float64).reshape(-1, 3)
    return float(np.linalg.norm(v.max(0) - v.min(0)))


def _set_camera(pkg, r, scene, eye, w, h):
    cam = scene.camera
    U, V, W = pkg.camera_frame(eye, cam["lookat"], cam["up"], cam["fov"], w / h)
    eye = np.array(eye, np.float32)
    r.set_camera(eye, U, V, W)
    return eye, U, V, W


def _film(r):
    """Everything the history calls must not write: film, frame and both feature planes, as bytes."""
    return tuple(a.tobytes() for a in (r.read_accum(), r.read_frame()) + tuple(r.read_features()))


def _weighted(R):
    R = np.asarray(R, np.float64)
    return np.concatenate([R[..., :3] * R[..., 3:4], R[..., 3:4]], -1)


# ------------------------------------------------------------------------------------------- the passes themselves, and chaining
@pytest.fixture(scope="module", params=[(48, 32), (43, 29)], ids=["48x32", "43x29"])
def moved(request, gpu, pkg, hip_lib):
    """4 frames of "pt" at camera A, captured; camera B = A orbited 20 degrees about the look-at point and dollied in by 10 %; one frame,
    the features, the prior, resolve(1), a second frame, resolve(2).  Every plane read back after every step.
    (An orbit of 5 degrees uncovers 1.0 / 1.4 % of the Cornell box's covered pixels in the float64 reference, 10 degrees 2.5 / 2.1 %,
    15 degrees 7.2 / 9.5 %; 20 degrees gives 16.7 / 13.9 % with m = 0 and 75.3 / 70.1 % with m > 3 at the two sizes.)"""
    assert hip_lib.spcbpt_build_arithmetic().decode() == "ieee"
    w, h = request.param
    scene = pkg.scenes.cornell_box()
    cam = scene.camera
    r = _renderer(pkg, scene, w, h)
    d = dict(r=r, w=w, h=h, sigma_x=SIGMA_X_FRACTION * _diag(scene), untouched=[])

    def history_call(fn, *a):
        before = _film(r)
        fn(*a)
        d["untouched"].append((fn.__name__, before == _film(r)))

    d["cam_a"] = _set_camera(pkg, r, scene, cam["eye"], w, h)
    for f in range(4):
        r.launch("pt", f)
        if f == 0:
            r.launch_features(0)
    d["accum_a"], (_, d["nd_a"]) = r.read_accum().copy(), r.read_features()
    history_call(r.history_capture, 4)
    d["history"] = r.read_history(False, False, False, True)["history"]
    lookat = np.asarray(cam["lookat"], np.float64)
    eye_b = lookat + 0.9 * (rr.orbit(cam["eye"], lookat, 20.0) - lookat)
    d["cam_b"] = _set_camera(pkg, r, scene, eye_b, w, h)
    r.launch("pt", 0)
    r.launch_features(0)
    d["nd_b"] = r.read_features()[1].copy()
    history_call(r.history_reproject, SIGMA_N, d["sigma_x"], MAX_HISTORY)
    for k in (1, 2):
        if k == 2:
            r.launch("pt", 1)
        history_call(r.history_resolve, k)
        d[f"accum_{k}"] = r.read_accum().copy()
        out = r.read_history(True, True, True, False)
        d[f"resolved_{k}"], d[f"frame_{k}"], d[f"prior_{k}"] = out["resolved"], out["frame"], out["prior"]
    return d


def test_device_prior_matches_formula_and_host(pkg, moved):
    d = moved
    prior = d["prior_1"]
    assert np.isfinite(prior).all() and np.array_equal(prior, d["prior_2"])
    args = (d["cam_b"], d["nd_b"], d["cam_a"], d["nd_a"], d["history"], SIGMA_N, d["sigma_x"], MAX_HISTORY)
    ref = _weighted(rr.reproject_ref(*args))
    host = _weighted(pkg.api.history_reproject_host(*args))
    top = ref.max()
    d_ref, d_host = np.abs(_weighted(prior) - ref).max() / top, np.abs(_weighted(prior) - host).max() / top
    covered = d["nd_b"][..., 3] > 0
    m = prior[..., 3][covered]
    ref_m = ref[..., 3][covered]
    print(f"{d['w']}x{d['h']}: prior, device - float64 {d_ref:.3g}, device - host {d_host:.3g} (of the largest m rgb {top:.3g}); of {int(covered.sum())} covered "
          f"pixels {100 * (m == 0).mean():.1f} % have m = 0 and {100 * (m > 3).mean():.1f} % m > 3 (float64: {100 * (ref_m == 0).mean():.1f} %, {100 * (ref_m > 3).mean():.1f} %)")
    assert d_ref <= BAR and d_host <= BAR
    assert (prior[~covered] == 0).all()
    # the history is the 4-frame film with n = 4 (no prior was live at the capture)
    assert d["history"][..., :3].tobytes() == d["accum_a"][..., :3].tobytes() and (d["history"][..., 3] == 4).all()
    # the move uncovers something and keeps most of the view
    assert (m == 0).mean() >= 0.05 and (m > 3).mean() >= 0.40
    assert all(ok for _, ok in d["untouched"]), d["untouched"]      # film, frame and features: byte for byte what they were


@pytest.mark.parametrize("frames", [1, 2])
def test_device_resolve_matches_formula_and_host(pkg, moved, frames):
    d = moved
    res, res8, prior, acc = d[f"resolved_{frames}"], d[f"frame_{frames}"], d[f"prior_{frames}"], d[f"accum_{frames}"]
    ref = rr.resolve_ref(prior, acc, frames)
    host = pkg.api.history_resolve_host(prior, acc, frames)
    top = ref[..., :3].max()
    d_ref, d_host = np.abs(res[..., :3] - ref[..., :3]).max() / top, np.abs(res[..., :3].astype(np.float64) - host[..., :3]).max() / top
    print(f"{d['w']}x{d['h']}: resolve({frames}), device - float64 {d_ref:.3g}, device - host {d_host:.3g} (of the largest channel {top:.3g})")
    assert np.isfinite(res).all()
    assert d_ref <= BAR and d_host <= BAR
    assert np.array_equal(res[..., 3], prior[..., 3] + np.float32(frames))
    assert np.abs(res[..., :3] - acc[..., :3]).max() > 1e-3                  # the prior counts
    # the RGBA8 plane is the film's tone map of the float plane: +-1 code where the float64 value sits at a quantisation tie
    codes = tone_map_codes(res[..., :3])
    want = np.minimum(np.floor(codes), 255)
    diff = res8[..., :3].astype(np.int64) - want
    tie = np.abs(codes - np.round(codes)) < 1e-3
    assert (res8[..., 3] == 255).all()
    assert (diff[~tie] == 0).all() and (np.abs(diff) <= 1).all(), (np.abs(diff).max(), int((diff != 0).sum()))


def test_chaining(pkg, moved):
    """A capture after resolve(2) keeps exactly what was shown, prior folded in, and ends the prior.  (Runs after the comparisons above:
    it changes the fixture's context, not its read-backs.)"""
    r = moved["r"]
    before = _film(r)
    r.history_capture(2)
    assert r.read_history(False, False, False, True)["history"].tobytes() == moved["resolved_2"].tobytes()
    with pytest.raises(pkg.SpcbptError) as e:
        r.read_history(False, False, True, False)
    assert f"({STATE})" in str(e.value) and "prior" in str(e.value)
    assert before == _film(r)
    r.history_resolve(2)                                                      # without a live prior: the film itself
    out = r.read_history()
    assert out["resolved"][..., :3].tobytes() == moved["accum_2"][..., :3].tobytes() and (out["resolved"][..., 3] == 2).all()


def test_errors(gpu, pkg):
    scene = pkg.scenes.cornell_box()
    w, h = 48, 32

    def fails(fn, code, text):
        with pytest.raises(pkg.SpcbptError) as e:
            fn()
        assert f"({code})" in str(e.value) and text in str(e.value), str(e.value)

    r = pkg.Renderer(scene, 0)
    cam = scene.camera
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
    for fn in (lambda: r.history_capture(1), lambda: r.history_reproject(), lambda: r.history_resolve(1)):
        fails(fn, STATE, "before spcbpt_resize")
    r.resize(w, h)
    r.launch("pt", 0)
    fails(lambda: r.history_capture(1), STATE, "feature")                    # before any feature launch
    fails(lambda: r.history_reproject(), STATE, "feature")
    fails(lambda: r.read_history(), STATE, "resolve")
    r.history_resolve(1)                                                     # needs neither features nor a history: the film itself
    assert r.read_history()["resolved"][..., :3].tobytes() == r.read_accum()[..., :3].tobytes()
    r.launch_features(0)
    fails(lambda: r.history_reproject(), STATE, "captured history")          # reproject before capture
    fails(lambda: r.history_capture(0), INVALID, "frames")
    fails(lambda: r.history_resolve(0), INVALID, "frames")
    r.launch_deferred("pt", 1)
    for fn in (lambda: r.history_capture(1), lambda: r.history_reproject(), lambda: r.history_resolve(1)):
        fails(fn, STATE, "deferred")
    r.merge_deferred(True)
    r.history_capture(2)
    for bad in ((float("nan"), 0, 0), (0, float("nan"), 0), (0, 0, float("nan"))):
        fails(lambda: r.history_reproject(*bad), INVALID, "not a number")
    r.history_reproject()
    r.history_resolve(2)
    out = r.read_history(True, True, True, True)
    assert all(np.isfinite(a).all() for a in out.values()) and out["prior"][..., 3].max() > 1
    r.clear_accum()                                                          # leaves the history alone
    assert r.read_history(False, False, False, True)["history"].tobytes() == out["history"].tobytes()
    r.history_reset()
    for which in ((True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True)):
        fails(lambda: r.read_history(*which), STATE, "read_history")
    fails(lambda: r.history_reproject(), STATE, "captured history")
    r.launch("pt", 0)
    r.history_capture(1)
    r.resize(w, h)                                                           # a resize forgets features, history and results
    r.launch("pt", 0)
    r.launch_features(0)
    fails(lambda: r.history_reproject(), STATE, "captured history")
    fails(lambda: r.read_history(False, False, False, True), STATE, "capture")


# ------------------------------------------------------------------------------------------------------------ what it is for
def test_resolved_image_is_closer_to_the_reference_after_a_move(gpu, pkg):
    """Cornell box at 64 x 64: 64 frames of "pt" at A, captured; orbit by 2 degrees to B; the resolved image after 1 and after 4 frames
    at B is closer (RMSE) to a disjoint 512-frame "pt" mean at B than the film is.  16 and 64 frames are printed."""
    scene = pkg.scenes.cornell_box()
    cam = scene.camera
    w = h = 64
    r = _renderer(pkg, scene, w, h)
    for f in range(64):
        r.launch("pt", f)
        if f == 0:
            r.launch_features(0)
    r.history_capture(64)
    _set_camera(pkg, r, scene, rr.orbit(cam["eye"], cam["lookat"], 2.0), w, h)
    shots = {}
    for f in range(64 + 512):
        r.launch("pt", f)
        if f == 0:
            r.launch_features(0)
            r.history_reproject()
        if f + 1 in (1, 4, 16, 64):
            r.history_resolve(f + 1)
            shots[f + 1] = (r.read_accum().copy(), r.read_history()["resolved"].copy())
    total = r.read_accum()[..., :3].astype(np.float64)
    reference = (576 * total - 64 * shots[64][0][..., :3].astype(np.float64)) / 512        # frames 64 .. 575: disjoint from every shot
    ratios = {}
    for k, (film, resolved) in shots.items():
        ratios[k] = (_rmse(film, reference), _rmse(resolved, reference))
    print("cornell 64x64, orbit 2 degrees after 64 frames; RMSE film -> resolved (ratio): " +
          ", ".join(f"{k} frames {a:.4f} -> {b:.4f} ({b / a:.3f})" for k, (a, b) in ratios.items()))
    assert ratios[1][1] < ratios[1][0]
    assert ratios[4][1] < ratios[4][0]


# ------------------------------------------------------------------------------------------------------------ the viewer
W_V, H_V = 48, 32


def _viewer_run(pkg, scene, mode, reproject):
    """6 steady frames of "pt", a left-button drag, one frame, 2 steady frames.  reproject: None = the switch is never touched,
    False = switched on and off again before the first frame, True = on.  Returns the renderer, the viewer and per shown frame
    (subframe index, live, film bytes, resolved plane or None, camera)."""
    cam = scene.camera
    r = _renderer(pkg, scene, W_V, H_V)
    v = pkg.api.Viewer(r, cam["eye"], cam["lookat"], cam["up"], cam["fov"], W_V, H_V)
    v.set_fps(60.0)
    if mode != 2:
        v.set_pipeline(mode)
    if reproject is not None:
        v.set_reproject(True)
        if not reproject:
            v.set_reproject(False)
    v.key("SPACE")
    assert v.state()["alg"] == "pt"
    shots = []

    def show(n):
        for _ in range(n):
            v.frame()
            st = v.state()
            res = r.read_history()["resolved"].copy() if reproject else None
            shots.append((st["subframe_index"], v.get_reproject()["live"], r.read_accum().tobytes(), res, (st["eye"], st["U"], st["V"], st["W"])))

    show(6)
    assert v.get_reproject()["live"] == 0
    v.mouse_button("left", 1, 10, 10); v.cursor_pos(22, 14); v.mouse_button("left", 0, 22, 14)
    show(1)
    assert v.get_reproject()["live"] == (1 if reproject else 0)
    show(2)
    return r, v, shots


def test_viewer_carries_the_image_across_a_drag(gpu, pkg):
    scene = pkg.scenes.cornell_box()
    runs = {}
    for mode in (0, 1, 2):
        r, v, shots = _viewer_run(pkg, scene, mode, True)
        runs[mode] = shots
        v.close(); r.close()
    assert [s[0] for s in runs[2]] == [1, 2, 3, 4, 5, 6, 1, 2, 3] and [s[1] for s in runs[2]] == [0] * 6 + [1] * 3
    # the same calls by hand on a second context
    b = _renderer(pkg, scene, W_V, H_V)
    by_hand = []
    b.set_camera(*runs[2][0][4])
    for f in range(6):
        b.launch("pt", f)
        if f == 0:
            b.launch_features(0)
        b.history_resolve(f + 1)
        by_hand.append(b.read_history()["resolved"].copy())
    b.history_capture(6)
    b.set_camera(*runs[2][6][4])
    for f in range(3):
        b.launch("pt", f)
        if f == 0:
            b.launch_features(0)
            b.history_reproject()
        b.history_resolve(f + 1)
        by_hand.append(b.read_history()["resolved"].copy())
    for k, want in enumerate(by_hand):
        for mode in (0, 1, 2):
            assert runs[mode][k][3].tobytes() == want.tobytes(), (k, mode)
            assert runs[mode][k][:2] == runs[2][k][:2], (k, mode)
    # before the drag the resolved image is the film; after it the prior shows
    film = [np.frombuffer(s[2], np.float32).reshape(H_V, W_V, 4) for s in runs[2]]
    assert all(by_hand[k][..., :3].tobytes() == film[k][..., :3].tobytes() for k in range(6))
    assert all(np.abs(by_hand[k][..., :3] - film[k][..., :3]).max() > 1e-3 for k in (6, 7, 8))
    # the film never hears of the switch: off again, or never touched, or on -- the same bytes after every frame, in every mode
    r, v, plain = _viewer_run(pkg, scene, 2, None)
    v.close(); r.close()
    for mode in (0, 1, 2):
        r, v, off = _viewer_run(pkg, scene, mode, False)
        v.close(); r.close()
        for k in range(len(plain)):
            assert off[k][2] == plain[k][2] and off[k][0] == plain[k][0] and off[k][1] == 0, (k, mode)
            assert runs[mode][k][2] == plain[k][2], (k, mode)


def test_viewer_tool_writes_resolved_frames(gpu, pkg, tmp_path):
    """tools/spcbpt_viewer --reproject on the Cornell box's .scene file with a three-event drag: exit 0; the frame written before the
    drag is the film's tone map, the one written after it is not (the film's tone map: the same session without --reproject)."""
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "spcbpt_viewer"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    path = pkg.scenes.write_scene(pkg.scenes.cornell_box(), str(tmp_path), "cornell")
    images = {}
    for name, flags in (("film", []), ("resolved", ["--reproject"])):
        script = os.path.join(str(tmp_path), name + ".script")
        with open(script, "w") as f:
            f.write(f"key SPACE\nfps 60\nframes 6\nsave {tmp_path}/{name}_before\npress left 10 10\nmove 22 14\nrelease left 22 14\nframes 2\nsave {tmp_path}/{name}_after\n")
        cmd = [os.path.join(ROOT, "tools", "spcbpt_viewer"), path, str(tmp_path), "--dim=48x32", "--minimal", "--script", script] + flags
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-3000:]
        for when in ("before", "after"):
            raw = open(f"{tmp_path}/{name}_{when}.ppm", "rb").read()
            assert raw.startswith(b"P6\n48 32\n255\n") and len(raw) == len(b"P6\n48 32\n255\n") + 48 * 32 * 3
            images[name, when] = raw
    assert images["resolved", "before"] == images["film", "before"]
    assert images["resolved", "after"] != images["film", "after"]
    a, b = (np.frombuffer(images[n, "after"][-48 * 32 * 3:], np.uint8).astype(np.int64) for n in ("resolved", "film"))
    print(f"tool: {int((a != b).sum())} of {a.size} bytes of the frame after the drag differ from the film's tone map")
