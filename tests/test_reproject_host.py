"""spcbpt_history_reproject_host / spcbpt_history_resolve_host -- the per-pixel functions the reprojection's kernels run
(csrc/reproject_pixel.h), on the host -- against the float64 restatement of the formula in include/spcbpt.h (tests/reproject_ref.py)
on an analytic scene.  Needs no GPU.

The scene: a wall z = 0 and a floor y = 0 (x in 0 .. 556), and an occluding rectangle at z = 150 over [180, 380] x [120, 330].  The
history camera sits at (278, 273, 800) and looks at (278, 273, 100); the current camera is orbited 6 degrees about that point from
650 away and raised to y = 300, so the occluder uncovers a strip of wall.  Features are ray-cast in float64 and rounded to float32.

Bar of the comparison with float64: 1e-4 of the plane's largest value, the denoiser's bar.  The formula itself, evaluated in float32
by tests/reproject_ref.py, deviates a few 1e-6 from its float64 evaluation on these inputs (printed), so the bar sits well over
rounding and no pixel is left out."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import reproject_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(48, 32), (43, 29)]
DIAG = float(np.sqrt(556.0 ** 2 + 556.0 ** 2 + 559.2 ** 2))
SIGMA_N, SIGMA_X, MAX_HISTORY = 0.25, 0.005 * DIAG, 32.0
BAR = 1e-4
LOOKAT, FOV = (278.0, 273.0, 100.0), 40.0
MISS, WALL, FLOOR, OCCLUDER = 0, 1, 2, 3
# the history image: per channel a + b sin(k . X + phase), a smooth function of the world position
IMAGE = [(0.5, 0.4, (1 / 90.0, 0.0, 0.0), 0.0), (0.5, 0.4, (0.0, 1 / 70.0, 0.0), 1.2), (0.5, 0.3, (1 / 110.0, 0.0, 1 / 110.0), 0.4)]


def image_at(X):
    X = np.asarray(X, np.float64)
    return np.stack([a + b * np.sin(X @ np.array(k) + ph) for a, b, k, ph in IMAGE], -1)


def cameras(w, h):
    hist = rr.lookat_camera((278.0, 273.0, 800.0), LOOKAT, (0, 1, 0), FOV, w / h)
    eye = rr.orbit((278.0, 273.0, 800.0), LOOKAT, 6.0, distance=650.0, y=300.0)
    return rr.lookat_camera(eye, LOOKAT, (0, 1, 0), FOV, w / h), hist


def ray_cast(cam, w, h):
    """(normal_depth float32 (h, w, 4), surface id (h, w)): the first hit of every pixel's centre ray, in float64."""
    eye, U, V, W = (np.asarray(v, np.float64) for v in cam)
    d = rr.centre_rays(U, V, W, w, h)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    best, sid = np.full((h, w), np.inf), np.zeros((h, w), np.int64)
    normal = np.zeros((h, w, 3))
    with np.errstate(all="ignore"):
        for s, (axis, level, n, inside) in {
                WALL: (2, 0.0, (0, 0, 1), lambda X: (X[..., 0] >= 0) & (X[..., 0] <= 556) & (X[..., 1] >= 0) & (X[..., 1] <= 556)),
                FLOOR: (1, 0.0, (0, 1, 0), lambda X: (X[..., 0] >= 0) & (X[..., 0] <= 556) & (X[..., 2] >= 0) & (X[..., 2] <= 2000)),
                OCCLUDER: (2, 150.0, (0, 0, 1), lambda X: (X[..., 0] >= 180) & (X[..., 0] <= 380) & (X[..., 1] >= 120) & (X[..., 1] <= 330))}.items():
            t = (level - eye[axis]) / d[..., axis]
            X = eye + d * t[..., None]
            hit = (t > 0) & np.isfinite(t) & inside(X) & (t < best)
            best, sid = np.where(hit, t, best), np.where(hit, s, sid)
            normal[hit] = n
    nd = np.zeros((h, w, 4), np.float32)
    nd[..., :3] = normal
    nd[..., 3] = np.where(sid > 0, best, 0.0)
    return nd, sid


def surface_constants(s):
    """(unit normal n, k): the plane n . X = k of surface s."""
    return {WALL: ((0.0, 0.0, 1.0), 0.0), FLOOR: ((0.0, 1.0, 0.0), 0.0), OCCLUDER: ((0.0, 0.0, 1.0), 150.0)}[s]


@pytest.fixture(scope="module", params=SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def case(request, pkg, hip_lib):
    w, h = request.param
    cur, hist = cameras(w, h)
    nd, sid = ray_cast(cur, w, h)
    G, sid_h = ray_cast(hist, w, h)
    H = np.zeros((h, w, 4), np.float32)
    H[..., :3] = image_at(rr.positions(hist, G)) * (sid_h > 0)[..., None]
    H[..., 3] = 64.0
    ref, det = rr.reproject_ref(cur, nd, hist, G, H, SIGMA_N, SIGMA_X, MAX_HISTORY, details=True)
    keep = [a.copy() for a in (nd, G, H)]
    host = pkg.api.history_reproject_host(cur, nd, hist, G, H, SIGMA_N, SIGMA_X, MAX_HISTORY)
    for a, k in zip((nd, G, H), keep):   # the inputs are not written
        assert np.array_equal(a, k)
    # which surface each of the four taps of a pixel lies on in the history view (-1: outside the image), from the float64 evaluation
    taps = np.full((h, w, 4), -1, np.int64)
    for t, (i, j) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        qx, qy = det["x0"] + i, det["y0"] + j
        inside = det["live"] & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
        taps[..., t] = np.where(inside, sid_h[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)], -1)
    return dict(w=w, h=h, cur=cur, hist=hist, nd=nd, sid=sid, G=G, sid_h=sid_h, H=H, ref=ref, det=det, host=host, taps=taps)


def _weighted(R):
    R = np.asarray(R, np.float64)
    return np.concatenate([R[..., :3] * R[..., 3:4], R[..., 3:4]], -1)


def test_host_matches_float64_formula(case):
    """(a) m rgb and m against the float64 restatement, no pixel left out."""
    ref, host = _weighted(case["ref"]), _weighted(case["host"])
    f32 = _weighted(rr.reproject_ref(case["cur"], case["nd"], case["hist"], case["G"], case["H"], SIGMA_N, SIGMA_X, MAX_HISTORY, dtype=np.float32))
    top = ref.max()
    dev, dev32 = np.abs(host - ref).max() / top, np.abs(f32 - ref).max() / top
    print(f"{case['w']}x{case['h']}: host - float64 {dev:.3g}, float32 formula - float64 {dev32:.3g} (of the largest value {top:.3g})")
    assert np.isfinite(case["host"]).all()
    assert dev <= BAR
    assert (case["host"][..., 3] > 3).mean() > 0.4 and top > 16     # the case is not empty


def test_identity(case, pkg):
    """(b) the history camera is the current camera: every covered pixel finds itself."""
    cur, nd, sid = case["cur"], case["nd"], case["sid"]
    H = np.zeros_like(case["H"])
    H[..., :3] = image_at(rr.positions(cur, nd)) * (sid > 0)[..., None]
    H[..., 3] = 64.0
    R = pkg.api.history_reproject_host(cur, nd, cur, nd, H, SIGMA_N, SIGMA_X, MAX_HISTORY)
    cov = sid > 0
    S = R[..., 3].astype(np.float64) / MAX_HISTORY           # N / S = 64 > max_history everywhere, so m = 32 S
    print(f"{case['w']}x{case['h']}: identity, smallest S {S[cov].min():.7f}, largest |rgb - history| {np.abs(R[..., :3] - H[..., :3])[cov].max():.3g}")
    assert cov.sum() > cov.size // 2
    assert (S[cov] >= 1 - 1e-5).all() and (S[cov] <= 1 + 1e-5).all()         # m = 32
    assert np.abs(R[..., :3].astype(np.float64) - H[..., :3])[cov].max() <= 1e-5
    assert (R[~cov] == 0).all()


def test_disocclusion_and_same_surface(case):
    """(c) wall pixels whose four history taps all lie on the occluder get no history at all; pixels whose four taps lie on their own
    surface get all of it."""
    sid, taps, host = case["sid"], case["taps"], case["host"]
    uncovered = (sid == WALL) & (taps == OCCLUDER).all(-1)
    same = (sid > 0) & (taps == sid[..., None]).all(-1)
    S = host[..., 3].astype(np.float64) / MAX_HISTORY
    print(f"{case['w']}x{case['h']}: {int(uncovered.sum())} disoccluded wall pixels, {int(same.sum())} same-surface pixels, smallest S there {S[same].min():.7f}")
    assert uncovered.sum() >= 8 and same.sum() >= 500
    assert (host[uncovered] == 0).all()
    assert (S[same] >= 1 - 1e-4).all()


def test_interpolation_error_is_bounded(case):
    """(d) on the same-surface pixels rgb is the bilinear interpolant of the history image over the tap cell, so it misses the analytic
    image at P by at most (max |g_uu| + max |g_vv|) / 8, g(u, v) = image(X(u, v)) over the cell in history pixel coordinates.  On the
    plane n . X = k seen from eye e along D(u, v) = dx U + dy V + W (affine in u, v; D_u = 2 U / w), with K = k - n . e:
        X_u  = K A_u / (n . D)^2,              A_u = (n . D) D_u - (n . D_u) D     (affine in u, v: its norm peaks at a corner)
        X_uu = -2 K (n . D_u) A_u / (n . D)^3
    and 1 / |n . D| peaks at a corner too, so both are bounded by corner values.  For a channel a + b sin(k . X + phase):
        |g_uu| <= b |k|^2 |X_u|^2 + b |k| |X_uu|.
    On top: the weights are b_q exp(-tiny) with exp >= 1 - 1e-4 (asserted in (c)), which moves the normalised weights by <= 1e-4 each,
    i.e. the result by <= 4e-4 of the image's range (below 1), and float32 rounding: (a)'s bar, which for m = 32 is 1e-4 of rgb."""
    w, h, sid, taps, det = case["w"], case["h"], case["sid"], case["taps"], case["det"]
    same = (sid > 0) & (taps == sid[..., None]).all(-1)
    eye, U, V, W = (np.asarray(v, np.float64) for v in case["hist"])
    bound = np.zeros((h, w, 3))
    for s in (WALL, FLOOR, OCCLUDER):
        n, k = surface_constants(s)
        n = np.array(n)
        K = k - n @ eye
        m = same & (sid == s)
        corners = []
        for i in (0, 1):
            for j in (0, 1):
                dx = 2.0 * ((det["x0"] + i + 0.5) / w) - 1.0
                dy = 2.0 * ((det["y0"] + j + 0.5) / h) - 1.0
                corners.append(dx[..., None] * U + dy[..., None] * V + W)
        nD = np.stack([c @ n for c in corners])                                   # (4, h, w)
        inv = (1.0 / np.abs(np.where(m, nD, 1.0))).max(0)
        for Ds, channel_bound in ((2.0 * U / w, None), (2.0 * V / h, None)):
            A = np.stack([np.linalg.norm((c @ n)[..., None] * Ds - (n @ Ds) * c, axis=-1) for c in corners]).max(0)
            X1 = abs(K) * A * inv ** 2
            X2 = 2.0 * abs(K) * abs(n @ Ds) * A * inv ** 3
            for ch, (a, b, kv, ph) in enumerate(IMAGE):
                kn = np.linalg.norm(kv)
                bound[..., ch] += np.where(m, (b * kn ** 2 * X1 ** 2 + b * kn * X2) / 8.0, 0.0)
    slack = 4e-4 * 1.0 + BAR
    want = image_at(det["P"])
    err = np.abs(case["host"][..., :3].astype(np.float64) - want)
    print(f"{w}x{h}: interpolation error on {int(same.sum())} same-surface pixels: largest {err[same].max():.4f}, largest bound {bound[same].max():.4f}, "
          f"smallest margin {(bound + slack - err)[same].min():.4f}")
    assert same.sum() >= 500
    assert (err[same] <= bound[same] + slack).all()
    assert bound[same].max() < 0.2      # the bound says something: the image's range is 0.8


def test_resolve_host(pkg, hip_lib):
    """(e) the blend's formula; one frame without a prior is the film bit for bit; NULL and frames = 0 are refused."""
    rng = np.random.default_rng(3)
    acc = rng.gamma(2.0, 0.4, size=(29, 43, 4)).astype(np.float32)
    acc[..., 3] = 1.0
    prior = rng.gamma(2.0, 0.4, size=(29, 43, 4)).astype(np.float32)
    prior[..., 3] = rng.uniform(0, 32, size=(29, 43)).astype(np.float32)
    prior[::3, ::2] = 0.0
    for frames in (1, 2, 7, 64):
        out = pkg.api.history_resolve_host(prior, acc, frames)
        ref = rr.resolve_ref(prior, acc, frames)
        assert np.abs(out - ref).max() <= 1e-6 * ref.max(), frames
        assert np.array_equal(out[..., 3], prior[..., 3] + np.float32(frames))
    one = pkg.api.history_resolve_host(None, acc, 1)
    assert one[..., :3].tobytes() == acc[..., :3].tobytes() and (one[..., 3] == 1).all()
    zero_prior = pkg.api.history_resolve_host(np.zeros_like(acc), acc, 1)
    assert zero_prior.tobytes() == one.tobytes()
    five = pkg.api.history_resolve_host(None, acc, 5)
    assert np.abs(five[..., :3] / acc[..., :3] - 1).max() <= 2e-7 and (five[..., 3] == 5).all()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros_like(acc)
    n = acc.size // 4
    assert hip_lib.spcbpt_history_resolve_host(fp(prior), fp(acc), 3, n, fp(out)) == 0
    assert hip_lib.spcbpt_history_resolve_host(fp(prior), None, 3, n, fp(out)) == -1
    assert hip_lib.spcbpt_history_resolve_host(fp(prior), fp(acc), 3, n, None) == -1
    assert hip_lib.spcbpt_history_resolve_host(fp(prior), fp(acc), 0, n, fp(out)) == -1
    assert hip_lib.spcbpt_history_resolve_host(fp(prior), fp(acc), 3, 0, fp(out)) == -1
    with pytest.raises(pkg.SpcbptError, match=r"\(-1\)"):
        pkg.api.history_resolve_host(prior, acc, 0)


def test_reproject_host_arguments(case, pkg, hip_lib):
    """Defaults for parameters <= 0, NaN and NULL refused, the struct's size."""
    cur, hist, nd, G, H = (case[k] for k in ("cur", "hist", "nd", "G", "H"))
    a = pkg.api.history_reproject_host(cur, nd, hist, G, H, diag=DIAG)
    b = pkg.api.history_reproject_host(cur, nd, hist, G, H, -1.0, 0.0, -3.0, diag=DIAG)
    assert np.array_equal(a, b) and np.isfinite(a).all() and a[..., 3].max() > 1
    for bad in ((np.nan, 1.0, 1.0), (1.0, np.nan, 1.0), (1.0, 1.0, np.nan)):
        with pytest.raises(pkg.SpcbptError, match=r"\(-1\)"):
            pkg.api.history_reproject_host(cur, nd, hist, G, H, *bad)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros_like(nd)
    p = pkg.api.ReprojectParams(SIGMA_N, SIGMA_X, MAX_HISTORY)
    args = [fp(v) for v in cur] + [fp(nd)] + [fp(v) for v in hist] + [fp(G), fp(H), case["w"], case["h"], C.byref(p), C.c_float(0.0), fp(out)]
    assert hip_lib.spcbpt_history_reproject_host(*args) == 0
    assert np.array_equal(out, case["host"])
    for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13, 15):
        bad = list(args)
        bad[k] = None
        assert hip_lib.spcbpt_history_reproject_host(*bad) == -1, k
    assert hip_lib.spcbpt_reproject_params_struct_size() == C.sizeof(pkg.api.ReprojectParams) == 12
    sizes = (C.c_int32 * 32)()
    assert hip_lib.spcbpt_abi_struct_sizes(sizes, 32) == 13


def test_native_program_under_sanitizers(pkg, hip_lib, tmp_path):
    """tests/native/reproject_check.cpp -- the two host forms in a program of its own, every plane in a heap block of its exact size --
    built with AddressSanitizer and UndefinedBehaviorSanitizer and run on the CPU at 43 x 29: no report, and the bits of the library's
    own host forms."""
    w, h = 43, 29
    exe, fin, fout = (str(tmp_path / n) for n in ("reproject_check", "in.bin", "out.bin"))
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "native", "reproject_check.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    cur, hist = cameras(w, h)
    nd, _ = ray_cast(cur, w, h)
    G, sid_h = ray_cast(hist, w, h)
    H = np.zeros((h, w, 4), np.float32)
    H[..., :3] = image_at(rr.positions(hist, G)) * (sid_h > 0)[..., None]
    H[..., 3] = 64.0
    acc = np.random.default_rng(5).gamma(2.0, 0.4, size=(h, w, 4)).astype(np.float32)
    with open(fin, "wb") as f:
        for a in tuple(cur) + tuple(hist) + (np.array([SIGMA_N, SIGMA_X, MAX_HISTORY], np.float32), nd, G, H, acc):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    r = subprocess.run([exe, fin, fout, str(w), str(h)], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    prior, res, film = np.fromfile(fout, np.float32).reshape(3, h, w, 4)
    want = pkg.api.history_reproject_host(cur, nd, hist, G, H, SIGMA_N, SIGMA_X, MAX_HISTORY)
    ref = _weighted(rr.reproject_ref(cur, nd, hist, G, H, SIGMA_N, SIGMA_X, MAX_HISTORY))
    assert np.abs(_weighted(prior) - ref).max() <= BAR * ref.max()
    assert np.array_equal(prior, want)
    assert np.array_equal(res, pkg.api.history_resolve_host(want, acc, 3))
    assert film[..., :3].tobytes() == acc[..., :3].tobytes()
