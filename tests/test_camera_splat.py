"""spcbpt_camera_splat -- the projection and importance the light-tracing estimator "lt" splats with -- against float64, without a
GPU: the exported entry is the host instantiation of the function the splat kernel calls (csrc/camera_splat.h)."""
import numpy as np
import pytest

W, H = 48, 32
# a modest eye position on purpose: the points handed over are float32, and a point 0.1 away from an eye at |eye| ~ 1 is rounded by
# 6e-8 / 0.1 of its offset -- far below the 0.01-pixel margins used here (at |eye| ~ 1000 the INPUT rounding alone would move it by more)
EYE = np.array([0.3, 0.4, 0.9], np.float32)
DISTANCES = (0.1, 3.0, 400.0)
JITTER = ((0.01, 0.01), (0.99, 0.01), (0.01, 0.99), (0.99, 0.99), (0.5, 0.5))


def _truth(eye, U, V, Wv, w, h, p):
    """float64: the 3 x 3 solve c = g (dx U + dy V + W), pixel and the reciprocal solid angle of a pixel along c."""
    eye, U, V, Wv, p = (np.asarray(a, np.float64) for a in (eye, U, V, Wv, p))
    c = p - eye
    M = np.stack([U, V, Wv], 1)
    a = np.linalg.solve(M, c.T).T
    g = a[..., 2]
    dx, dy = a[..., 0] / g, a[..., 1] / g
    q = c / g[..., None]
    we = w * h * np.linalg.norm(q, axis=-1) ** 3 / (4 * abs(np.linalg.det(M)))
    return dx, dy, g, we


def _round_trip(pkg, hip_lib, U, V, Wv):
    """Every pixel x five sub-pixel positions x three distances along the camera_ray direction: returns the largest |dx|, |dy| error
    against the generating values and the largest relative weight error against float64 (of the float32 point handed over)."""
    U64, V64, W64 = (np.asarray(a, np.float64) for a in (U, V, Wv))
    worst_d, worst_w, n = 0.0, 0.0, 0
    for y in range(H):
        for x in range(W):
            for jx, jy in JITTER:
                dx0, dy0 = 2 * (x + jx) / W - 1, 2 * (y + jy) / H - 1
                d = dx0 * U64 + dy0 * V64 + W64
                d /= np.linalg.norm(d)
                for t in DISTANCES:
                    p = (EYE.astype(np.float64) + t * d).astype(np.float32)
                    got = pkg.api.camera_splat(EYE, U, V, Wv, W, H, p)
                    assert got is not None, (x, y, jx, jy, t)
                    dx, dy, px, py, we = got
                    assert (px, py) == (x, y), (x, y, jx, jy, t, got)
                    _, _, _, we64 = _truth(EYE, U, V, Wv, W, H, p[None, :])
                    worst_d = max(worst_d, abs(dx - dx0), abs(dy - dy0))
                    worst_w = max(worst_w, abs(we / we64[0] - 1))
                    n += 1
    assert n == W * H * len(JITTER) * len(DISTANCES)
    return worst_d, worst_w


def test_round_trip_of_camera_ray(pkg, hip_lib):
    """A point on the ray camera_ray shoots through (x + jx, y + jy) comes back to pixel (x, y) with the generating (dx, dy) to 1e-5
    and the float64 weight to rtol 2.8e-6.  Measured: |dx|, |dy| error 8.5e-7 at most (float32 points 0.1 .. 400 from the eye), weight
    6.8e-7 relative -- its bar is that times 4 (the budget before measuring, six FP32 roundings of a cubic stated generously, was 1e-5)."""
    cam = pkg.scenes.cornell_box().camera
    U, V, Wv = pkg.camera_frame(EYE, EYE + (np.array(cam["lookat"], np.float32) - np.array(cam["eye"], np.float32)), cam["up"], cam["fov"], W / H)
    worst_d, worst_w = _round_trip(pkg, hip_lib, U, V, Wv)
    print(f"orthogonal frame: max |d - d0| {worst_d:.3g}, max relative weight error {worst_w:.3g}")
    assert worst_d <= 1e-5
    assert worst_w <= 2.8e-6


def test_round_trip_with_a_skewed_frame(pkg, hip_lib):
    """The same with a frame that is neither orthogonal nor normalised; the truth is the float64 3 x 3 solve.  Measured: 8.9e-7 in
    dx, dy, 8.3e-7 relative in the weight; the weight's bar is 4 x that."""
    U = np.array([1.3, 0.2, 0.0], np.float32)
    V = np.array([0.1, 0.8, 0.1], np.float32)
    Wv = np.array([0.2, -0.1, -2.0], np.float32)
    worst_d, worst_w = _round_trip(pkg, hip_lib, U, V, Wv)
    print(f"skewed frame: max |d - d0| {worst_d:.3g}, max relative weight error {worst_w:.3g}")
    assert worst_d <= 1e-5
    assert worst_w <= 3.4e-6


def test_points_that_must_not_splat(pkg, hip_lib):
    import ctypes as C
    U, V, Wv = pkg.camera_frame(EYE, EYE + np.array([0.0, 0.0, -1.0], np.float32), (0, 1, 0), 35.0, W / H)
    U64, V64, W64 = (np.asarray(a, np.float64) for a in (U, V, Wv))
    e = EYE.astype(np.float64)
    eps = 1e-4
    cases = {
        "behind": e - 2.0 * W64 + 0.1 * U64,
        "far behind": e - 300.0 * W64,
        "eye plane": e + 0.7 * U64 - 0.2 * V64,        # g = 0 exactly: U and V have no component along W here
        "the eye": e,
        "left": e + 3.0 * (-(1 + eps) * U64 + 0.3 * V64 + W64),
        "right": e + 3.0 * ((1 + eps) * U64 + 0.3 * V64 + W64),
        "below": e + 3.0 * (0.3 * U64 - (1 + eps) * V64 + W64),
        "above": e + 3.0 * (0.3 * U64 + (1 + eps) * V64 + W64),
    }
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    for name, p in cases.items():
        p32 = np.asarray(p, np.float32)
        assert pkg.api.camera_splat(EYE, U, V, Wv, W, H, p32) is None, name
        # nothing is written
        dx, dy, we = C.c_float(-7.0), C.c_float(-7.0), C.c_float(-7.0)
        px, py = C.c_int(-7), C.c_int(-7)
        rc = hip_lib.spcbpt_camera_splat(fp(EYE), fp(U), fp(V), fp(Wv), W, H, fp(p32), C.byref(dx), C.byref(dy), C.byref(px), C.byref(py), C.byref(we))
        assert rc == 0 and (dx.value, dy.value, we.value, px.value, py.value) == (-7.0, -7.0, -7.0, -7, -7), name
    # just inside each border it does splat, into the border pixel
    for name, (ax, ay, want) in {"left": (-(1 - eps), 0.3, (0, None)), "right": (1 - eps, 0.3, (W - 1, None)),
                                 "below": (0.3, -(1 - eps), (None, 0)), "above": (0.3, 1 - eps, (None, H - 1))}.items():
        got = pkg.api.camera_splat(EYE, U, V, Wv, W, H, np.asarray(e + 3.0 * (ax * U64 + ay * V64 + W64), np.float32))
        assert got is not None, name
        assert (want[0] is None or got[2] == want[0]) and (want[1] is None or got[3] == want[1]), (name, got)
    # the largest float below 1 in dx: (dx + 1) rounds to 2, and the pixel stays inside the image
    got = pkg.api.camera_splat(np.zeros(3, np.float32), np.array([1, 0, 0], np.float32), np.array([0, 1, 0], np.float32), np.array([0, 0, -1], np.float32),
                               W, H, np.array([np.nextafter(np.float32(1), np.float32(0)), 0.0, -1.0], np.float32))
    assert got is not None and got[2] == W - 1


@pytest.mark.parametrize("skewed", [False, True])
def test_the_weight_integrates_to_the_radiance(pkg, hip_lib, skewed):
    """A plane patch that faces the camera and fills the frustum, radiating 1: the sum over the patch of cos_b / |c|^2 x weight x [the
    point lands in the pixel] dA is the pixel's value, 1.  Midpoint rule on 400 x 400 cells per pixel footprint in float64, with the
    library's own weight and pixel checked on a 20 x 20 sub-grid of every footprint; 12 pixels including the corners.  A wrong power of the cosine, a missing aspect factor
    or a w / h mix-up misses 1 by per cents, the bar is 1e-3."""
    if skewed:
        U, V, Wv = np.array([1.3, 0.2, 0.0], np.float32), np.array([0.1, 0.8, 0.1], np.float32), np.array([0.2, -0.1, -2.0], np.float32)
    else:
        U, V, Wv = pkg.camera_frame(EYE, EYE + np.array([0.2, -0.1, -1.0], np.float32), (0, 1, 0), 50.0, W / H)
    U64, V64, W64 = (np.asarray(a, np.float64) for a in (U, V, Wv))
    e = EYE.astype(np.float64)
    # the patch: the plane through eye + 2.5 W spanned by U and V (it contains every pixel's footprint); its normal faces the camera
    dist = 2.5
    n = np.cross(U64, V64)
    n /= np.linalg.norm(n)
    if n @ W64 > 0:
        n = -n
    cell_area = np.linalg.norm(np.cross(U64, V64)) * (2 * dist / W) * (2 * dist / H)    # of a pixel footprint on the patch
    N = 400
    s = (np.arange(N) + 0.5) / N
    pixels = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2), (1, H // 2), (W - 2, 3), (7, 5), (20, 30), (33, 11), (40, 17), (13, 24)]
    assert len(pixels) == 12
    worst = 0.0
    rng = np.random.default_rng(5)
    for x, y in pixels:
        dx = 2 * (x + s) / W - 1
        dy = 2 * (y + s) / H - 1
        P = e + dist * (dx[None, :, None] * U64 + dy[:, None, None] * V64 + W64)      # (N, N, 3) midpoints of the cells
        c = P - e
        r2 = (c * c).sum(-1)
        cosb = -(c @ n) / np.sqrt(r2)
        assert (cosb > 0).all()
        # the library's weight varies smoothly over a footprint: evaluated (float32) on a 20 x 20 sub-grid of the cells and at random
        # cells for the pixel test, and in float64 (checked against the library to 3.4e-6 by the round-trip tests) everywhere
        _, _, _, we = _truth(EYE, U, V, Wv, W, H, P.reshape(-1, 3))
        we = we.reshape(N, N)
        for iy in list(range(10, N, 20)):
            for ix in range(10, N, 20):
                got = pkg.api.camera_splat(EYE, U, V, Wv, W, H, P[iy, ix].astype(np.float32))
                assert got is not None and (got[2], got[3]) == (x, y), (x, y, ix, iy, got)
                assert abs(got[4] / we[iy, ix] - 1) < 1e-5
        total = (cosb / r2 * we).sum() * cell_area / (N * N)
        worst = max(worst, abs(total - 1))
        # and a point of the neighbouring footprints does NOT land in this pixel
        for ox, oy in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            xn, yn = x + ox, y + oy
            if 0 <= xn < W and 0 <= yn < H:
                jx, jy = rng.uniform(0.05, 0.95, 2)
                p = e + dist * ((2 * (xn + jx) / W - 1) * U64 + (2 * (yn + jy) / H - 1) * V64 + W64)
                got = pkg.api.camera_splat(EYE, U, V, Wv, W, H, p.astype(np.float32))
                assert got is not None and (got[2], got[3]) == (xn, yn)
    print(f"{'skewed' if skewed else 'orthogonal'} frame: max |integral - 1| over 12 pixels {worst:.3g}")
    assert worst <= 1e-3
