"""The variance the history carries and the denoiser on the resolved image, on the device (spcbpt_history_denoise,
spcbpt_read_history_variance): HV, PV and RV against the float64 restatement of the formulas (tests/history_var_ref.py) and against
the host forms, all run on the device's own read-back planes, under the project's bar (1e-4 of the compared plane's largest value:
tests/test_history_variance_host.py; the library under test is the IEEE build); the outputs the variance-carrying kernels share with
the plain ones byte for byte; the filter; the two bit identities; the state errors; what the feature is for -- the first frames after a
camera move closer to a converged image than the resolved image is; the viewer's switch in its three pipeline modes, and
tools/spcbpt_viewer --reproject --denoise.

Measured on the MI355X: see DESIGN.md 8g."""
import os
import subprocess

import numpy as np
import pytest

from tests import history_var_ref as hv
from tests import reproject_ref as rr
from tests.denoise_ref import tone_map_codes
from tests.test_gpu_mesh_light import _renderer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-4
STATE, INVALID = -5, -1
SIGMA_N, SIGMA_X_FRACTION, MAX_HISTORY = 0.25, 0.005, 32.0
DN_SIGMA = (4.0, 0.5, 0.2)


def _rmse(a, b, mask=None):
    d = (np.asarray(a, np.float64)[..., :3] - np.asarray(b, np.float64)[..., :3]) ** 2
    return float(np.sqrt(np.mean(d if mask is None else d[mask])))


def _diag(scene):
    v = np.asarray(scene.vertices, np.float64).reshape(-1, 3)
    return float(np.linalg.norm(v.max(0) - v.min(0)))


def _set_camera(pkg, r, scene, eye, w, h):
    cam = scene.camera
    U, V, W = pkg.camera_frame(eye, cam["lookat"], cam["up"], cam["fov"], w / h)
    eye = np.array(eye, np.float32)
    r.set_camera(eye, U, V, W)
    return eye, U, V, W


def _film(r, moments):
    """Everything the history calls must not write: film, frame, both feature planes and the moments, as bytes."""
    planes = (r.read_accum(), r.read_frame()) + tuple(r.read_features()) + ((r.read_film_moments(),) if moments else ())
    return tuple(a.tobytes() for a in planes)


def _m2(prior, var):
    """m^2 PV: the quantity the resolve consumes."""
    m = np.asarray(prior, np.float64)[..., 3:4]
    return m * m * np.asarray(var, np.float64)[..., :3]


# ------------------------------------------------------------------------------------------- the passes themselves, and chaining
def _moved_sequence(pkg, w, h, moments):
    """tests/test_gpu_reproject.py's sequence: 4 frames of "pt" at camera A, captured; camera B = A orbited 20 degrees about the look-at
    point and dollied in by 10 %; one frame, the features, the prior, resolve(1), a second frame, resolve(2).  Every plane read back
    after every step; with the moments on also the variance planes, and after resolve(1) the history denoiser at 1 and 5 iterations."""
    scene = pkg.scenes.cornell_box()
    cam = scene.camera
    r = _renderer(pkg, scene, w, h)
    r.set_film_moments(moments)
    d = dict(r=r, w=w, h=h, sigma_x=SIGMA_X_FRACTION * _diag(scene), untouched=[])

    def history_call(fn, *a):
        before = _film(r, moments)
        fn(*a)
        d["untouched"].append((fn.__name__, before == _film(r, moments)))

    d["cam_a"] = _set_camera(pkg, r, scene, cam["eye"], w, h)
    for f in range(4):
        r.launch("pt", f)
        if f == 0:
            r.launch_features(0)
    d["accum_a"], (_, d["nd_a"]) = r.read_accum().copy(), r.read_features()
    if moments:
        d["m2n_a"] = r.read_film_moments().copy()
    history_call(r.history_capture, 4)
    d["history"] = r.read_history(False, False, False, True)["history"]
    if moments:
        d["hv"] = r.read_history_variance(False, False, True)["history"]
    lookat = np.asarray(cam["lookat"], np.float64)
    eye_b = lookat + 0.9 * (rr.orbit(cam["eye"], lookat, 20.0) - lookat)
    d["cam_b"] = _set_camera(pkg, r, scene, eye_b, w, h)
    r.launch("pt", 0)
    r.launch_features(0)
    d["alb_b"], d["nd_b"] = (a.copy() for a in r.read_features())
    history_call(r.history_reproject, SIGMA_N, d["sigma_x"], MAX_HISTORY)
    for k in (1, 2):
        if k == 2:
            r.launch("pt", 1)
        history_call(r.history_resolve, k)
        d[f"accum_{k}"] = r.read_accum().copy()
        out = r.read_history(True, True, True, False)
        d[f"resolved_{k}"], d[f"frame_{k}"], d[f"prior_{k}"] = out["resolved"], out["frame"], out["prior"]
        if moments:
            d[f"m2n_{k}"] = r.read_film_moments().copy()
            var = r.read_history_variance(True, True, False)
            d[f"rv_{k}"], d[f"pv_{k}"] = var["resolved"], var["prior"]
            if k == 1:
                for it in (1, 5):
                    history_call(r.history_denoise, it, *DN_SIGMA)
                    d[f"denoised_{it}"], d[f"denoised8_{it}"] = (a.copy() for a in r.read_denoised())
                after = r.read_history(True, True, True, False)               # the filter writes the denoiser's planes only
                d["history_planes_kept"] = all(after[n].tobytes() == out[n].tobytes() for n in out) and \
                    all(a.tobytes() == b.tobytes() for a, b in zip(r.read_history_variance(True, True, True).values(), (var["resolved"], var["prior"], d["hv"])))
    return d


@pytest.fixture(scope="module", params=[(48, 32), (43, 29)], ids=["48x32", "43x29"])
def moved(request, gpu, pkg, hip_lib):
    assert hip_lib.spcbpt_build_arithmetic().decode() == "ieee"
    w, h = request.param
    d = _moved_sequence(pkg, w, h, True)
    off = _moved_sequence(pkg, w, h, False)
    d["off"] = {k: v for k, v in off.items() if k != "r"}
    off["r"].close()
    return d


def test_variance_planes_match_formula_and_host(pkg, moved):
    d = moved
    # HV after the first capture: VA of the 4-frame film, the host form's bits
    _, va = pkg.api.history_resolve_var_host(None, None, d["accum_a"], d["m2n_a"], 4)
    assert (d["m2n_a"][..., 3] == 4).all()
    assert d["hv"].tobytes() == va.tobytes()
    ref = hv.film_variance_ref(d["accum_a"], d["m2n_a"])
    assert np.abs(d["hv"][..., :3] - ref).max() <= BAR * ref.max() and ref.max() > 0
    # PV, as m^2 PV
    args = (d["cam_b"], d["nd_b"], d["cam_a"], d["nd_a"], d["history"])
    prior, pv = d["prior_1"], d["pv_1"]
    assert np.isfinite(pv).all() and np.array_equal(pv, d["pv_2"]) and (pv[..., 3] == 0).all()
    ref_prior, ref_pv = hv.prior_variance_ref(*args, d["hv"], SIGMA_N, d["sigma_x"], MAX_HISTORY)
    host_prior, host_pv = pkg.api.history_reproject_var_host(*args, d["hv"], SIGMA_N, d["sigma_x"], MAX_HISTORY)
    ref = _m2(ref_prior, ref_pv)
    top = ref.max()
    d_ref, d_host = np.abs(_m2(prior, pv) - ref).max() / top, np.abs(_m2(prior, pv) - _m2(host_prior, host_pv)).max() / top
    print(f"{d['w']}x{d['h']}: m^2 PV, device - float64 {d_ref:.3g}, device - host {d_host:.3g} (of the largest value {top:.3g})")
    assert d_ref <= BAR and d_host <= BAR and top > 0
    dead = (prior == 0).all(-1)
    assert (pv[dead] == 0).all() and dead.sum() >= 8                          # PV is zero wherever R is: misses and uncovered pixels
    assert (pv[~dead][..., :3].max(-1) > 0).mean() > 0.9
    # RV after one and after two frames
    for k in (1, 2):
        rv = d[f"rv_{k}"]
        ref = hv.resolve_variance_ref(d[f"prior_{k}"], pv, d[f"accum_{k}"], d[f"m2n_{k}"], k)
        _, host = pkg.api.history_resolve_var_host(d[f"prior_{k}"], pv, d[f"accum_{k}"], d[f"m2n_{k}"], k)
        top = ref.max()
        d_ref, d_host = np.abs(rv[..., :3] - ref).max() / top, np.abs(rv[..., :3].astype(np.float64) - host[..., :3]).max() / top
        print(f"{d['w']}x{d['h']}: RV({k}), device - float64 {d_ref:.3g}, device - host {d_host:.3g} (of the largest value {top:.3g})")
        assert np.isfinite(rv).all() and (rv[..., 3] == 0).all()
        assert d_ref <= BAR and d_host <= BAR
        assert (d[f"m2n_{k}"][..., 3] == k).all()                             # k = 1: the unknown-variance line, k = 2: the moments' own


def test_variance_carrying_kernels_do_not_move_the_existing_outputs(moved):
    """Prior, resolved image and RGBA8 frame: byte for byte what the same sequence gives with the moments off; film, frame, features
    and moments: untouched by every history call, the new ones included."""
    d, off = moved, moved["off"]
    for k in ("history", "prior_1", "prior_2", "resolved_1", "resolved_2", "frame_1", "frame_2", "accum_1", "accum_2"):
        assert d[k].tobytes() == off[k].tobytes(), k
    assert all(ok for _, ok in d["untouched"]), d["untouched"]
    assert [n for n, _ in d["untouched"]].count("history_denoise") == 2
    assert d["history_planes_kept"]


@pytest.mark.parametrize("iterations", [1, 5])
def test_device_filter_matches_formula_and_host(pkg, moved, iterations):
    d = moved
    out, out8 = d[f"denoised_{iterations}"], d[f"denoised8_{iterations}"]
    eye, U, V, W = d["cam_b"]
    ref = hv.history_denoise_ref(d["resolved_1"], d["rv_1"], d["alb_b"], d["nd_b"], U, V, W, iterations, *DN_SIGMA)
    host = pkg.api.history_denoise_host(d["resolved_1"], d["rv_1"], d["alb_b"], d["nd_b"], eye, U, V, W, iterations, *DN_SIGMA)
    top = ref.max()
    d_ref, d_host = np.abs(out[..., :3] - ref).max() / top, np.abs(out[..., :3].astype(np.float64) - host[..., :3]).max() / top
    print(f"{d['w']}x{d['h']}: history denoise, {iterations} iterations: device - float64 {d_ref:.3g}, device - host {d_host:.3g} (of the largest channel {top:.3g})")
    assert np.isfinite(out).all() and (out[..., 3] == 1).all()
    assert d_ref <= BAR and d_host <= BAR
    assert np.abs(out[..., :3] - d["resolved_1"][..., :3]).max() > 1e-3       # it filtered
    # the RGBA8 plane is the film's tone map of the float plane: +-1 code where the float64 value sits at a quantisation tie
    codes = tone_map_codes(out[..., :3])
    want = np.minimum(np.floor(codes), 255)
    diff = out8[..., :3].astype(np.int64) - want
    tie = np.abs(codes - np.round(codes)) < 1e-3
    assert (out8[..., 3] == 255).all()
    assert (diff[~tie] == 0).all() and (np.abs(diff) <= 1).all(), (np.abs(diff).max(), int((diff != 0).sum()))


def test_capture_keeps_the_resolved_variance(pkg, moved):
    """A capture after resolve(2) makes HV the RV just read, byte for byte, and ends the prior and its variance.  (Runs after the
    comparisons above: it changes the fixture's context, not its read-backs.)"""
    r = moved["r"]
    before = _film(r, True)
    r.history_capture(2)
    assert r.read_history_variance(False, False, True)["history"].tobytes() == moved["rv_2"].tobytes()
    assert r.read_history(False, False, False, True)["history"].tobytes() == moved["resolved_2"].tobytes()
    with pytest.raises(pkg.SpcbptError) as e:
        r.read_history_variance(False, True, False)
    assert f"({STATE})" in str(e.value) and "prior" in str(e.value)
    assert before == _film(r, True)


def test_without_a_prior_it_is_denoise_variance_bit_for_bit(gpu, pkg):
    """4 frames, no capture, resolve(4): every pixel has n = 4 and no prior is live -- history_denoise and denoise_variance return the
    same bytes."""
    scene = pkg.scenes.cornell_box()
    for w, h in ((48, 32), (43, 29)):
        r = _renderer(pkg, scene, w, h)
        r.set_film_moments(True)
        for f in range(4):
            r.launch("pt", f)
            if f == 0:
                r.launch_features(0)
        r.history_resolve(4)
        assert (r.read_film_moments()[..., 3] == 4).all()
        for args in ((1,) + DN_SIGMA, (5,) + DN_SIGMA, ()):
            r.history_denoise(*args)
            a = [x.copy() for x in r.read_denoised()]
            r.denoise_variance(*args)
            b = r.read_denoised()
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), (w, h, args)
        assert np.abs(a[0][..., :3] - r.read_accum()[..., :3]).max() > 1e-3
        r.close()


# ------------------------------------------------------------------------------------------------------------ states
def test_errors(gpu, pkg):
    scene = pkg.scenes.cornell_box()
    w, h = 48, 32

    def fails(fn, code, text):
        with pytest.raises(pkg.SpcbptError) as e:
            fn()
        assert f"({code})" in str(e.value) and text in str(e.value), str(e.value)

    r = _renderer(pkg, scene, w, h)
    r.set_film_moments(True)
    r.launch("pt", 0)
    fails(lambda: r.history_denoise(), STATE, "feature")                      # without features
    r.launch_features(0)
    fails(lambda: r.history_denoise(), STATE, "resolve")                      # before any resolve
    fails(lambda: r.read_history_variance(), STATE, "resolve")
    r.set_film_moments(False)
    r.launch("pt", 0)
    r.history_resolve(1)
    fails(lambda: r.history_denoise(), STATE, "moments were off")             # with the moments off
    fails(lambda: r.read_history_variance(), STATE, "moments were off")
    r.history_capture(1)                                                      # a capture made with the moments off ...
    fails(lambda: r.read_history_variance(False, False, True), STATE, "moments were off")
    r.set_film_moments(True)
    r.launch("pt", 0)
    r.history_reproject()
    r.history_resolve(1)                                                      # ... followed by reproject and resolve with them on
    fails(lambda: r.history_denoise(), STATE, "moments were off at the capture or resolve")
    fails(lambda: r.read_history_variance(False, True, False), STATE, "moments were off")
    assert np.isfinite(r.read_history()["resolved"]).all()                    # the resolve itself is what it always was
    r.history_capture(1)                                                      # no variance came in: none goes out
    fails(lambda: r.read_history_variance(False, False, True), STATE, "moments were off")
    r.history_resolve(1)                                                      # the capture ended the prior: the film's own variance
    r.history_denoise()
    for it in (0, 9):
        fails(lambda: r.history_denoise(it), INVALID, "iterations")
    for bad in ((float("nan"), 0, 0), (0, float("nan"), 0), (0, 0, float("nan"))):
        fails(lambda: r.history_denoise(5, *bad), INVALID, "not a number")
    r.launch_deferred("pt", 1)
    fails(lambda: r.history_denoise(), STATE, "deferred")                     # with a deferred frame outstanding
    r.merge_deferred(True)
    r.history_resolve(2)
    r.history_denoise()                                                       # the context stays usable
    assert all(np.isfinite(a).all() for a in r.read_denoised())
    assert np.isfinite(r.read_history_variance()["resolved"]).all()
    r.set_film_moments(False)                                                 # switching the moments off invalidates the variance planes
    fails(lambda: r.read_history_variance(), STATE, "read_history_variance")
    fails(lambda: r.history_denoise(), STATE, "moments were off")
    r.set_film_moments(True)
    r.launch("pt", 0)
    r.history_capture(1)
    r.history_reproject()
    r.history_resolve(1)
    assert all(np.isfinite(a).all() for a in r.read_history_variance(True, True, True).values())
    r.history_reset()                                                         # spcbpt_history_reset invalidates them
    for which in ((True, False, False), (False, True, False), (False, False, True)):
        fails(lambda: r.read_history_variance(*which), STATE, "read_history_variance")
    fails(lambda: r.history_denoise(), STATE, "resolve")
    r.history_capture(1)
    r.history_resolve(1)
    r.resize(w, h)                                                            # ... and so does spcbpt_resize
    r.launch("pt", 0)
    r.launch_features(0)
    for which in ((True, False, False), (False, False, True)):
        fails(lambda: r.read_history_variance(*which), STATE, "read_history_variance")
    fails(lambda: r.history_denoise(), STATE, "resolve")
    r.history_resolve(1)
    r.history_denoise()
    assert all(np.isfinite(a).all() for a in r.read_denoised())
    r.close()


# ------------------------------------------------------------------------------------------------------------ what it is for
def _after_a_move(pkg, degrees):
    """tests/test_gpu_reproject.py's scenario with the moments on: Cornell box at 64 x 64, 64 frames of "pt" at A, captured; an orbit;
    at 1, 4, 16 and 64 frames at B the film, the resolved image, its variance and the default history denoise; the reference is the
    disjoint mean of frames 64 .. 575 at B.  Returns (shots, reference, the prior's m)."""
    scene = pkg.scenes.cornell_box()
    cam = scene.camera
    w = h = 64
    r = _renderer(pkg, scene, w, h)
    r.set_film_moments(True)
    for f in range(64):
        r.launch("pt", f)
        if f == 0:
            r.launch_features(0)
    r.history_capture(64)
    _set_camera(pkg, r, scene, rr.orbit(cam["eye"], cam["lookat"], degrees), w, h)
    shots = {}
    for f in range(64 + 512):
        r.launch("pt", f)
        if f == 0:
            r.launch_features(0)
            r.history_reproject()
        if f + 1 in (1, 4, 16, 64):
            r.history_resolve(f + 1)
            r.history_denoise()
            shots[f + 1] = (r.read_accum().copy(), r.read_history()["resolved"].copy(), r.read_history_variance()["resolved"].copy(), r.read_denoised()[0].copy())
    m = r.read_history(False, False, True, False)["prior"][..., 3].copy()
    total = r.read_accum()[..., :3].astype(np.float64)
    reference = (576 * total - 64 * shots[64][0][..., :3].astype(np.float64)) / 512        # frames 64 .. 575: disjoint from every shot
    r.close()
    return shots, reference, m


def test_denoised_image_is_closer_to_the_reference_after_a_move(gpu, pkg):
    """After a 2 degree orbit the default history denoise is closer (RMSE) to the reference than the resolved image, at 1 and at 4
    frames at B: asserted.  Printed and not asserted (nobody has measured them before; a variance from 1 - 4 frames is heavy-tailed and
    the reference carries noise of its own): 16 and 64 frames, the same after a 20 degree orbit restricted to the pixels without a
    prior (m = 0), and the calibration ratio sum (resolved - reference)^2 / sum RV at 1, 4 and 16 frames."""
    shots, reference, _ = _after_a_move(pkg, 2.0)
    ratios = {k: (_rmse(film, reference), _rmse(res, reference), _rmse(den, reference)) for k, (film, res, _, den) in shots.items()}
    print("cornell 64x64, orbit 2 degrees after 64 frames; RMSE film -> resolved -> history denoise (denoised / resolved): " +
          ", ".join(f"{k} frames {a:.4f} -> {b:.4f} -> {c:.4f} ({c / b:.3f})" for k, (a, b, c) in ratios.items()))
    calib = {k: float(((shots[k][1][..., :3].astype(np.float64) - reference) ** 2).sum() / shots[k][2][..., :3].astype(np.float64).sum()) for k in (1, 4, 16)}
    print("calibration sum (resolved - reference)^2 / sum RV: " + ", ".join(f"{k} frames {v:.3f}" for k, v in calib.items()))
    shots20, reference20, m = _after_a_move(pkg, 20.0)
    fresh = m == 0
    print(f"orbit 20 degrees, the {int(fresh.sum())} pixels with m = 0; RMSE resolved -> history denoise: " +
          ", ".join(f"{k} frames {_rmse(res, reference20, fresh):.4f} -> {_rmse(den, reference20, fresh):.4f}" for k, (_, res, _, den) in shots20.items()))
    assert ratios[1][2] < ratios[1][1]
    assert ratios[4][2] < ratios[4][1]


# ------------------------------------------------------------------------------------------------------------ the viewer
W_V, H_V = 48, 32


def _viewer_run(pkg, scene, mode, denoise):
    """tests/test_gpu_reproject.py's session: 6 steady frames of "pt", a left-button drag, one frame, 2 steady frames.  denoise: None =
    neither switch is ever touched, True = reproject and denoise on.  Returns the renderer, the viewer and per shown frame (subframe
    index, film bytes, denoised planes as bytes or None, camera)."""
    cam = scene.camera
    r = _renderer(pkg, scene, W_V, H_V)
    v = pkg.api.Viewer(r, cam["eye"], cam["lookat"], cam["up"], cam["fov"], W_V, H_V)
    v.set_fps(60.0)
    if mode != 2:
        v.set_pipeline(mode)
    if denoise:
        v.set_reproject(True)
        v.set_denoise(True)
        assert v.get_denoise() and r.film_moments()
    v.key("SPACE")
    assert v.state()["alg"] == "pt"
    shots = []

    def show(n):
        for _ in range(n):
            v.frame()
            st = v.state()
            den = b"".join(a.tobytes() for a in r.read_denoised()) if denoise else None
            shots.append((st["subframe_index"], r.read_accum().tobytes(), den, (st["eye"], st["U"], st["V"], st["W"])))

    show(6)
    v.mouse_button("left", 1, 10, 10); v.cursor_pos(22, 14); v.mouse_button("left", 0, 22, 14)
    show(3)
    return r, v, shots


def test_viewer_denoises_what_it_shows(gpu, pkg):
    scene = pkg.scenes.cornell_box()
    runs = {}
    for mode in (0, 1, 2):
        r, v, shots = _viewer_run(pkg, scene, mode, True)
        runs[mode] = shots
        v.set_denoise(False)                                                  # switching it off restores the moments switch it found
        assert not v.get_denoise() and not r.film_moments() and v.get_reproject()["on"] == 1
        v.set_denoise(True)
        v.set_reproject(False)                                                # switching reproject off switches denoise off
        assert not v.get_denoise() and not r.film_moments()
        with pytest.raises(pkg.SpcbptError) as e:
            v.set_denoise(True)                                               # not without reproject
        assert f"({STATE})" in str(e.value)
        v.close(); r.close()
    assert [s[0] for s in runs[2]] == [1, 2, 3, 4, 5, 6, 1, 2, 3]
    # the same calls by hand on a second context
    b = _renderer(pkg, scene, W_V, H_V)
    b.set_film_moments(True)
    by_hand = []
    b.set_camera(*runs[2][0][3])
    for f in range(6):
        b.launch("pt", f)
        if f == 0:
            b.launch_features(0)
        b.history_resolve(f + 1)
        b.history_denoise()
        by_hand.append(b"".join(a.tobytes() for a in b.read_denoised()))
    b.history_capture(6)
    b.set_camera(*runs[2][6][3])
    for f in range(3):
        b.launch("pt", f)
        if f == 0:
            b.launch_features(0)
            b.history_reproject()
        b.history_resolve(f + 1)
        b.history_denoise()
        by_hand.append(b"".join(a.tobytes() for a in b.read_denoised()))
    b.close()
    for k, want in enumerate(by_hand):
        for mode in (0, 1, 2):
            assert runs[mode][k][2] == want, (k, mode)
            assert runs[mode][k][0] == runs[2][k][0], (k, mode)
    # the film never hears of either switch
    r, v, plain = _viewer_run(pkg, scene, 2, None)
    v.close(); r.close()
    for mode in (0, 1, 2):
        for k in range(len(plain)):
            assert runs[mode][k][1] == plain[k][1] and runs[mode][k][0] == plain[k][0], (k, mode)


def test_viewer_tool_writes_denoised_frames(gpu, pkg, tmp_path):
    """tools/spcbpt_viewer --reproject --denoise on the Cornell box's .scene file with a three-event drag: exit 0, and the frame written
    after the drag is not the --reproject-only frame; --denoise alone is a usage error."""
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "spcbpt_viewer"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    path = pkg.scenes.write_scene(pkg.scenes.cornell_box(), str(tmp_path), "cornell")
    tool = os.path.join(ROOT, "tools", "spcbpt_viewer")
    images = {}
    for name, flags in (("resolved", ["--reproject"]), ("denoised", ["--reproject", "--denoise"])):
        script = os.path.join(str(tmp_path), name + ".script")
        with open(script, "w") as f:
            f.write(f"key SPACE\nfps 60\nframes 6\npress left 10 10\nmove 22 14\nrelease left 22 14\nframes 2\nsave {tmp_path}/{name}_after\n")
        p = subprocess.run([tool, path, str(tmp_path), "--dim=48x32", "--minimal", "--script", script] + flags, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-3000:]
        raw = open(f"{tmp_path}/{name}_after.ppm", "rb").read()
        assert raw.startswith(b"P6\n48 32\n255\n") and len(raw) == len(b"P6\n48 32\n255\n") + 48 * 32 * 3
        images[name] = raw
    assert images["denoised"] != images["resolved"]
    a, b = (np.frombuffer(images[n][-48 * 32 * 3:], np.uint8).astype(np.int64) for n in ("denoised", "resolved"))
    print(f"tool: {int((a != b).sum())} of {a.size} bytes of the denoised frame after the drag differ from the resolved frame")
    p = subprocess.run([tool, path, str(tmp_path), "--dim=48x32", "--minimal", "--script", script, "--denoise"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 1 and "--reproject" in p.stdout
