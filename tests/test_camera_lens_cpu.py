"""The thin-lens camera's host forms (csrc/camera_lens.h through spcbpt_camera_lens_ray_host / spcbpt_camera_splat_lens) against the
float64 definition of tests/lens_ref.py.  Needs no GPU.

The accuracy bars are RUNNING ERROR BOUNDS of the definition evaluated naively in float32, not figures taken from the code: every
quantity is carried as (value, bound of its absolute error) through the definition's own expression,
    x (+-) y : e = e_x + e_y + eps |x (+-) y|          x y : e = |x| e_y + |y| e_x + eps |x y|
    x / y    : e = (e_x + |x / y| e_y) / |y| + eps |x / y|        sqrt x : e = e_x / (2 sqrt x) + eps sqrt x
with eps = 2^-24 (round to nearest), the camera's vectors and the inputs exact, and the two trigonometric values of the disc map good
to 2 ulp (what both libm and the device library promise, and what the header's polynomial kernels document).  The expression is the
definition's literal one -- F = eye + focus d, O = eye + R (a U^ + b V^), F - O; c = P - O, g, q, F = O + q, the projection of
F - eye -- so the bound contains the cancellations against |eye| and |P| that make up the conditioning.  The assertion is
err <= 4 x that bound, sample by sample ("floor over the conditioning", tests/connect_ref.py); the measured ratios are printed."""
import numpy as np
import pytest

from tests import lens_ref as L
from tests.lens_film import host_film
from tests.test_gpu_mesh_light import _chi2_sf

EPS = 2.0 ** -24
W_, H_ = 48, 32


def frames(pkg):
    """An orthogonal frame (the Cornell box's camera at 48 x 32) and a sheared, scaled one."""
    cam = pkg.scenes.cornell_box().camera
    U, V, W = pkg.camera_frame(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W_ / H_)
    eye = np.array(cam["eye"], np.float32)
    shear = (eye + np.float32(0.25), (U + np.float32(0.3) * W + np.float32(0.1) * V).astype(np.float32), (V * np.float32(1.2) - np.float32(0.2) * U).astype(np.float32),
             (W + np.float32(0.15) * U).astype(np.float32))
    return {"orthogonal": (eye, U, V, W), "sheared": shear}


# ---------------------------------------------------------------------------------------------- running error arithmetic
class E:
    def __init__(self, v, e=None):
        self.v = np.asarray(v, np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, np.float64)

    def _r(self, v, e):
        return E(v, e + EPS * np.abs(v))

    def __add__(self, o):
        o = o if isinstance(o, E) else E(o)
        return self._r(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = o if isinstance(o, E) else E(o)
        return self._r(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = o if isinstance(o, E) else E(o)
        return self._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    def __truediv__(self, o):
        o = o if isinstance(o, E) else E(o)
        v = self.v / o.v
        return self._r(v, (self.e + np.abs(v) * o.e) / np.abs(o.v))

    def sqrt(self):
        v = np.sqrt(self.v)
        return self._r(v, self.e / (2 * v))


def vec(a):
    return [E(a[..., k]) for k in range(3)]


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def lens_point_bound(eye, U, V, u1, u2, R):
    a, b = L.disc(u1, u2)
    # (a, b): the ratio, its product with pi / 4 (a rounded constant), a 2-ulp trigonometric value, the product with r: the angle is
    # off by <= 3 eps (pi / 4) and the kernel by 4 eps, so each coordinate by <= (3 pi / 4 + 4 + 1) eps < 8 eps of the unit disc
    a, b = E(a, 8 * EPS * np.ones_like(a)), E(b, 8 * EPS * np.ones_like(b))
    Uv, Vv = vec(np.asarray(U, np.float64)), vec(np.asarray(V, np.float64))
    ul, vl = dot(Uv, Uv).sqrt(), dot(Vv, Vv).sqrt()
    return [E(np.float64(eye[k])) + (a * (Uv[k] / ul) + b * (Vv[k] / vl)) * R for k in range(3)]


def ray_bound(eye, U, V, W, x, y, jx, jy, u1, u2, R, f):
    """-> (origin bound (n, 3), direction bound (n, 3)) of the naive float32 evaluation of the definition."""
    dx = (E(x) + E(jx)) / W_ * 2.0 - 1.0
    dy = (E(y) + E(jy)) / H_ * 2.0 - 1.0
    O = lens_point_bound(eye, U, V, u1, u2, R)
    F = [E(np.float64(eye[k])) + (dx * np.float64(U[k]) + dy * np.float64(V[k]) + np.float64(W[k])) * f for k in range(3)]
    d = [F[k] - O[k] for k in range(3)]
    ln = dot(d, d).sqrt()
    out = [d[k] / ln for k in range(3)]
    return np.stack([o.e for o in O], -1), np.stack([o.e for o in out], -1)


def splat_bound(eye, U, V, W, P, u1, u2, R, f):
    """-> bounds of (dx, dy, weight) for the naive float32 evaluation of the light side's definition."""
    O = lens_point_bound(eye, U, V, u1, u2, R)
    Uv, Vv, Wv = (vec(np.asarray(v, np.float64)) for v in (U, V, W))
    uv, vw, wu = cross(Uv, Vv), cross(Vv, Wv), cross(Wv, Uv)
    D = dot(Uv, vw)
    c = [E(P[..., k]) - O[k] for k in range(3)]
    g = dot(c, uv) / D
    q = [c[k] * (E(f) / g) for k in range(3)]
    Fe = [(O[k] + q[k]) - E(np.float64(eye[k])) for k in range(3)]
    gf = dot(Fe, uv) / D
    dx = (dot(Fe, vw) / D) / gf
    dy = (dot(Fe, wu) / D) / gf
    r = dot(q, q).sqrt()
    we = (r * r * r) * float(W_ * H_) / ((dot(q, uv) * (4.0 * f * f)))
    return dx.e, dy.e, we.e


def samples(rng, n):
    x, y = rng.integers(0, W_, n), rng.integers(0, H_, n)
    j = rng.random((n, 2)).astype(np.float32)
    u = (rng.integers(0, 1 << 24, (n, 2)) / float(1 << 24)).astype(np.float32)   # what rnd() returns: multiples of 2^-24
    return np.stack([x, y], 1).astype(np.int32), j, u


# ---------------------------------------------------------------------------------------------- radius 0
@pytest.mark.parametrize("name", ["orthogonal", "sheared"])
def test_radius_zero_is_the_pinhole_bit_for_bit(pkg, hip_lib, name):
    """radius = 0: the host ray is `eye` and camera_ray's direction -- dx U + dy V + W, then v * (1 / sqrt(v . v)), every operation in
    float32 in that order, recomputed here with numpy float32 -- and the host splat is spcbpt_camera_splat; `focus` is ignored."""
    eye, U, V, W = frames(pkg)[name]
    rng = np.random.default_rng(1)
    xy, j, u = samples(rng, 2000)
    f = np.float32
    for focus in (1.0, 3.0):
        o, d = pkg.api.camera_lens_ray_host(eye, U, V, W, W_, H_, xy, j, u, 0.0, focus)
        dx = (f(2.0) * ((xy[:, 0].astype(f) + j[:, 0]) / f(W_)) - f(1.0)).astype(f)
        dy = (f(2.0) * ((xy[:, 1].astype(f) + j[:, 1]) / f(H_)) - f(1.0)).astype(f)
        v = ((dx[:, None] * U[None, :]).astype(f) + (dy[:, None] * V[None, :]).astype(f)).astype(f)
        v = (v + W[None, :]).astype(f)
        n2 = ((v[:, 0] * v[:, 0]).astype(f) + (v[:, 1] * v[:, 1]).astype(f)).astype(f)
        n2 = (n2 + (v[:, 2] * v[:, 2]).astype(f)).astype(f)
        inv = (f(1.0) / np.sqrt(n2, dtype=f)).astype(f)
        want = (v * inv[:, None]).astype(f)
        assert d.tobytes() == want.tobytes()
        assert o.tobytes() == np.broadcast_to(eye, o.shape).astype(f).tobytes()
        O64, d64, _, _ = L.lens_ray(eye, U, V, W, W_, H_, xy[:, 0], xy[:, 1], j[:, 0], j[:, 1], u[:, 0], u[:, 1], 0.0, focus)
        pts = (O64 + rng.uniform(0.3, 4.0, (len(xy), 1)) * d64 * np.linalg.norm(W)).astype(f)
        pts[::7] = eye - (pts[::7] - eye)      # some behind the camera
        pts[::11] += f(3.0) * U                # ... and some outside the image
        inside, dxdy, pixel, weight = pkg.api.camera_splat_lens(eye, U, V, W, W_, H_, pts, u, 0.0, focus)
        assert 0.5 < inside.mean() < 0.95
        for i in range(len(pts)):
            s = pkg.api.camera_splat(eye, U, V, W, W_, H_, pts[i])
            assert (s is not None) == bool(inside[i])
            if s is not None:
                assert np.array([s[0], s[1], s[4]], f).tobytes() == np.array([dxdy[i, 0], dxdy[i, 1], weight[i]], f).tobytes()
                assert (s[2], s[3]) == (pixel[i, 0], pixel[i, 1])


# ---------------------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("name", ["orthogonal", "sheared"])
def test_host_ray_against_the_float64_definition(pkg, hip_lib, name):
    eye, U, V, W = frames(pkg)[name]
    R, focus = float(np.float32(0.03 * np.linalg.norm(W))), float(np.float32(0.7))
    xy, j, u = samples(np.random.default_rng(2), 10000)
    o, d = pkg.api.camera_lens_ray_host(eye, U, V, W, W_, H_, xy, j, u, R, focus)
    O64, d64, _, _ = L.lens_ray(eye, U, V, W, W_, H_, xy[:, 0], xy[:, 1], j[:, 0], j[:, 1], u[:, 0], u[:, 1], R, focus)
    bo, bd = ray_bound(eye, U, V, W, xy[:, 0], xy[:, 1], j[:, 0], j[:, 1], u[:, 0], u[:, 1], R, focus)
    eo, ed = np.abs(o - O64), np.abs(d - d64)
    print(f"{name}: host ray vs float64: origin {eo.max():.3g} (largest error / bound {np.max(eo / bo):.3f}), direction {ed.max():.3g} "
          f"(largest error / bound {np.max(ed / bd):.3f}); bounds up to {bo.max():.3g} / {bd.max():.3g}")
    assert (eo <= 4 * bo).all() and (ed <= 4 * bd).all()
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 4 * EPS


@pytest.mark.parametrize("name", ["orthogonal", "sheared"])
def test_host_splat_against_the_float64_definition(pkg, hip_lib, name):
    """Points at depths 0.3 .. 4 (units of W) along rays through the image and beyond its border.  Inside / outside agrees except within
    the bound of the border (and of the lens plane); dx, dy and the weight are held to 4 x their bounds; the pixel agrees unless the
    continuous coordinate lies within 4 x the bound of a pixel border."""
    eye, U, V, W = frames(pkg)[name]
    R, focus = float(np.float32(0.03 * np.linalg.norm(W))), float(np.float32(0.7))
    rng = np.random.default_rng(3)
    n = 10000
    u = (rng.integers(0, 1 << 24, (n, 2)) / float(1 << 24)).astype(np.float32)
    s, t = rng.uniform(-1.15, 1.15, (2, n))
    depth = rng.uniform(0.3, 4.0, n)
    P = (eye + depth[:, None] * (s[:, None] * U + t[:, None] * V + W)).astype(np.float32)
    inside, dxdy, pixel, weight = pkg.api.camera_splat_lens(eye, U, V, W, W_, H_, P, u, R, focus)
    ref = L.splat_lens(eye, U, V, W, W_, H_, P, u[:, 0], u[:, 1], R, focus)
    bx, by, bw = splat_bound(eye, U, V, W, P.astype(np.float64), u[:, 0], u[:, 1], R, focus)
    clear = (np.abs(np.abs(ref["dx"]) - 1) > 4 * bx) & (np.abs(np.abs(ref["dy"]) - 1) > 4 * by)
    assert (inside[clear] == ref["inside"][clear]).all()
    both = inside & ref["inside"]
    assert both.sum() > 6000
    ex, ey = np.abs(dxdy[both, 0] - ref["dx"][both]), np.abs(dxdy[both, 1] - ref["dy"][both])
    ew = np.abs(weight[both] - ref["weight"][both])
    print(f"{name}: host splat vs float64 on {int(both.sum())} points: dx {ex.max():.3g} (error / bound {np.max(ex / bx[both]):.3f}), dy {ey.max():.3g} "
          f"({np.max(ey / by[both]):.3f}), weight relative {np.max(ew / ref['weight'][both]):.3g} ({np.max(ew / bw[both]):.3f})")
    assert (ex <= 4 * bx[both]).all() and (ey <= 4 * by[both]).all() and (ew <= 4 * bw[both]).all()
    fx, fy = ref["fx"][both], ref["fy"][both]
    safe = (np.abs(fx - np.round(fx)) > 4 * bx[both] * W_ / 2) & (np.abs(fy - np.round(fy)) > 4 * by[both] * H_ / 2)
    assert safe.mean() > 0.99
    assert (pixel[both][safe, 0] == ref["px"][both][safe]).all() and (pixel[both][safe, 1] == ref["py"][both][safe]).all()


# ---------------------------------------------------------------------------------------------- round trip
@pytest.mark.parametrize("name", ["orthogonal", "sheared"])
def test_round_trip(pkg, hip_lib, name):
    """A point O + t dir of a generated ray, splatted with the same (u1, u2), lands on that ray's (dx, dy): the line from O through the
    point meets the plane in focus at the ray's own focus point, whatever t.  Held to 4 x the sum of the splat's bound and the bound of
    the point itself (it is rounded to float32: eps |P| across, seen at |q| / |c| magnification); the pixel is the ray's wherever the
    sample keeps that distance from a pixel border."""
    eye, U, V, W = frames(pkg)[name]
    R, focus = float(np.float32(0.03 * np.linalg.norm(W))), float(np.float32(0.7))
    rng = np.random.default_rng(4)
    xy, j, u = samples(rng, 4000)
    o, d = pkg.api.camera_lens_ray_host(eye, U, V, W, W_, H_, xy, j, u, R, focus)
    t = rng.uniform(0.3, 4.0, (len(xy), 1)) * np.linalg.norm(W)
    P = (o.astype(np.float64) + t * d.astype(np.float64)).astype(np.float32)
    inside, dxdy, pixel, weight = pkg.api.camera_splat_lens(eye, U, V, W, W_, H_, P, u, R, focus)
    _, _, dx, dy = L.lens_ray(eye, U, V, W, W_, H_, xy[:, 0], xy[:, 1], j[:, 0], j[:, 1], u[:, 0], u[:, 1], R, focus)
    bx, by, _ = splat_bound(eye, U, V, W, P.astype(np.float64), u[:, 0], u[:, 1], R, focus)
    _, bd = ray_bound(eye, U, V, W, xy[:, 0], xy[:, 1], j[:, 0], j[:, 1], u[:, 0], u[:, 1], R, focus)
    # a direction error e moves the focus point by |q| e, i.e. dx by about |q| e / (focus |U|); the rounding of P by eps |P| (|q| / |c|) / (focus |U|)
    ref = L.splat_lens(eye, U, V, W, W_, H_, P, u[:, 0], u[:, 1], R, focus)
    qn = np.linalg.norm(ref["origin"] - (eye + focus * (dx[:, None] * U + dy[:, None] * V + W)), axis=1)
    extra = (qn * bd.max(1) * 2 + EPS * np.linalg.norm(P, axis=1) * 2 * qn / (t[:, 0])) / (focus * min(np.linalg.norm(U), np.linalg.norm(V)) * abs(np.sin(_angle(U, V))))
    fx, fy = (dx + 1) / 2 * W_, (dy + 1) / 2 * H_
    tol_x, tol_y = 4 * (bx + extra), 4 * (by + extra)
    assert inside[(np.abs(np.abs(dx) - 1) > tol_x) & (np.abs(np.abs(dy) - 1) > tol_y)].all()
    ex, ey = np.abs(dxdy[inside, 0] - dx[inside]), np.abs(dxdy[inside, 1] - dy[inside])
    print(f"{name}: round trip dx {ex.max():.3g}, dy {ey.max():.3g} (largest error / tolerance {max(np.max(ex / tol_x[inside]), np.max(ey / tol_y[inside])):.3f})")
    assert (ex <= tol_x[inside]).all() and (ey <= tol_y[inside]).all()
    safe = inside & (np.abs(fx - np.round(fx)) > tol_x * W_ / 2) & (np.abs(fy - np.round(fy)) > tol_y * H_ / 2)
    assert safe.mean() > 0.99
    assert (pixel[safe, 0] == xy[safe, 0]).all() and (pixel[safe, 1] == xy[safe, 1]).all()


def _angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arccos(np.clip(a @ b / np.linalg.norm(a) / np.linalg.norm(b), -1, 1))


# ---------------------------------------------------------------------------------------------- in focus / circle of confusion
@pytest.mark.parametrize("name", ["orthogonal", "sheared"])
def test_in_focus_is_sharp_and_defocus_is_a_disc(pkg, hip_lib, name):
    """A point on the plane g = focus lands on one (dx, dy) for every lens sample.  A point P at depth g != focus spreads over a disc:
    with e = P - eye and o = O - eye (o in the lens plane, depth 0), F - eye = o + (focus / g)(e - o) = (focus / g) e + (1 - focus / g) o.
    The first term is the pinhole image of P; the second is the lens disc scaled by |1 - focus / g| -- similar triangles with apex P,
    bases on the lens plane and the plane in focus.  In (dx, dy) a displacement s U^ of the focus point is s / (focus |U|) when U and V
    are orthogonal, so the image of the lens rim is the ellipse with semi-axes
        R |1 - focus / g| / (focus |U|)  in dx   and   R |1 - focus / g| / (focus |V|)  in dy;
    for a sheared frame the displacement (1 - focus / g) o is decomposed in the (U, V) basis of the plane instead, which is what the
    test does for both.  Checked on the rim (u2 = 0 maps onto it: |(a, b)| = 1) and inside (every sample within the rim's ellipse)."""
    eye, U, V, W = frames(pkg)[name]
    R, focus = float(np.float32(0.03 * np.linalg.norm(W))), float(np.float32(0.7))
    rng = np.random.default_rng(5)
    n = 512
    u = (rng.integers(0, 1 << 24, (n, 2)) / float(1 << 24)).astype(np.float32)
    e64, U64, V64, W64 = (np.asarray(v, np.float64) for v in (eye, U, V, W))
    for g in (focus, 0.35, 2.5):
        P = (e64 + g * (0.21 * U64 - 0.33 * V64 + W64)).astype(np.float32)
        pts = np.broadcast_to(P, (n, 3)).copy()
        inside, dxdy, _, _ = pkg.api.camera_splat_lens(eye, U, V, W, W_, H_, pts, u, R, focus)
        assert inside.all()
        bx, by, _ = splat_bound(eye, U, V, W, pts.astype(np.float64), u[:, 0], u[:, 1], R, focus)
        gP, dx0, dy0 = L.project(eye, U, V, W, P.astype(np.float64))   # (the rounded point's own depth and pinhole image)
        k = 1 - focus / gP
        a, b = L.disc(u[:, 0], u[:, 1])
        disp = k * R * (a[:, None] * U64 / np.linalg.norm(U64) + b[:, None] * V64 / np.linalg.norm(V64))
        coef = np.linalg.lstsq(np.stack([U64, V64], 1), disp.T, rcond=None)[0].T / focus      # disp = focus (ddx U + ddy V)
        ex, ey = np.abs(dxdy[:, 0] - (dx0 + coef[:, 0])), np.abs(dxdy[:, 1] - (dy0 + coef[:, 1]))
        spread = np.ptp(dxdy, axis=0)
        print(f"{name}: depth {g:.2f}: spread of (dx, dy) over the lens {spread}, against the similar-triangle image {ex.max():.3g} / {ey.max():.3g}")
        assert (ex <= 4 * bx).all() and (ey <= 4 * by).all()
        if g == focus:
            assert spread.max() <= 8 * max(bx.max(), by.max())
        else:
            rim = 2 * abs(k) * R / (focus * max(np.linalg.norm(U64), np.linalg.norm(V64)))
            assert spread.min() > 0.5 * rim       # a disc of the derived size, not a point


# ---------------------------------------------------------------------------------------------- Jacobian
def test_weight_times_solid_angle_is_one(pkg, hip_lib):
    """weight x Omega = 1, Omega the solid angle, seen from the lens point, of the pixel's footprint on the plane in focus (float64, the
    footprint split into triangles: lens_ref.footprint_solid_angle).  The weight is a density at the pixel's centre and Omega an integral
    over the pixel, so they agree to second order in the pixel's angular size theta: at 2048 x 2048 theta < 1.2e-3 for these frames,
    theta^2 < 1.5e-6, and the bar is 1e-5.  The reference is checked first, then the host form against it, and the test proves that it
    can fail: lens_ref with camera_splat's pinhole weight (which measures |c / g| from the eye and on the plane g = 1) misses the bar."""
    w = h = 2048
    rng = np.random.default_rng(6)
    for name, (eye, U, V, W) in frames(pkg).items():
        R, focus = float(np.float32(0.05 * np.linalg.norm(W))), float(np.float32(0.7))
        n = 40
        px, py = rng.integers(0, w, n), rng.integers(0, h, n)
        u = (rng.integers(0, 1 << 24, (n, 2)) / float(1 << 24)).astype(np.float32)
        O, d, _, _ = L.lens_ray(eye, U, V, W, w, h, px, py, np.full(n, 0.5), np.full(n, 0.5), u[:, 0], u[:, 1], R, focus)
        P = O + rng.uniform(0.3, 4.0, (n, 1)) * np.linalg.norm(W) * d
        omega = np.array([L.footprint_solid_angle(eye, U, V, W, w, h, px[i], py[i], O[i], focus, n=2) for i in range(n)])
        ref = L.splat_lens(eye, U, V, W, w, h, P, u[:, 0], u[:, 1], R, focus)
        bad = L.splat_lens(eye, U, V, W, w, h, P, u[:, 0], u[:, 1], R, focus, pinhole_weight=True)
        assert ref["inside"].all() and (ref["px"] == px).all() and (ref["py"] == py).all()
        dev_ref, dev_bad = np.abs(ref["weight"] * omega - 1), np.abs(bad["weight"] * omega - 1)
        inside, _, pixel, weight = pkg.api.camera_splat_lens(eye, U, V, W, w, h, P.astype(np.float32), u, R, focus)
        assert inside.all()
        # (the host form sees the point rounded to float32: its weight is compared with the reference's AT that point, then with Omega)
        ref32 = L.splat_lens(eye, U, V, W, w, h, P.astype(np.float32), u[:, 0], u[:, 1], R, focus)
        dev_host = np.abs(weight / ref32["weight"] - 1)
        print(f"{name}: |weight x Omega - 1|: reference {dev_ref.max():.3g}, with the pinhole weight {dev_bad.max():.3g} (smallest {dev_bad.min():.3g}); "
              f"host weight against the reference {dev_host.max():.3g}")
        assert dev_ref.max() <= 1e-5
        assert dev_host.max() <= 1e-5
        assert dev_bad.max() > 1e-3, "the seeded corruption (the pinhole's weight) passes: the test cannot see a wrong Jacobian"


# ---------------------------------------------------------------------------------------------- disc map
def test_disc_map_is_uniform_and_stays_inside(pkg, hip_lib):
    """The host's disc map, read off the lens points of a unit frame (eye 0, U = x, V = y, R = 1: origin = (a, b, 0)).  Uniformity: chi^2
    over an 8 x 8 polar grid of equal areas (8 rings in r^2, 8 sectors) on 10^5 samples, tail probability above 1e-6 like the BSDF
    chi^2 tests; and against the float64 map to 8 eps.  The corners of the unit square (0 and 1 - 2^-24 in either place) stay finite
    and inside the disc -- up to the rounding of a point ON the rim (u = 0 maps to |r| = 1 exactly): 4 eps."""
    eye, U, V, W = (np.array(v, np.float32) for v in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)))
    rng = np.random.default_rng(7)
    n = 100000
    u = (rng.integers(0, 1 << 24, (n, 2)) / float(1 << 24)).astype(np.float32)
    xy = np.zeros((n, 2), np.int32)
    o, _ = pkg.api.camera_lens_ray_host(eye, U, V, W, 8, 8, xy, np.full((n, 2), 0.5, np.float32), u, 1.0, 1.0)
    assert (o[:, 2] == 0).all()
    a, b = o[:, 0].astype(np.float64), o[:, 1].astype(np.float64)
    ra, rb = L.disc(u[:, 0], u[:, 1])
    print(f"disc map against float64: {max(np.abs(a - ra).max(), np.abs(b - rb).max()):.3g}")
    assert np.abs(a - ra).max() <= 8 * EPS and np.abs(b - rb).max() <= 8 * EPS
    ring = np.minimum((8 * (a * a + b * b)).astype(int), 7)
    sector = np.minimum(((np.arctan2(b, a) + np.pi) / (2 * np.pi) * 8).astype(int), 7)
    counts = np.bincount(ring * 8 + sector, minlength=64).astype(np.float64)
    chi2 = ((counts - n / 64) ** 2 / (n / 64)).sum()
    p = _chi2_sf(chi2, 63)
    print(f"disc map uniformity: chi^2 = {chi2:.1f} with 63 degrees of freedom, tail probability {p:.3g}")
    assert p > 1e-6, chi2
    top = np.float32(1 - 2.0 ** -24)
    corners = np.array([(p, q) for p in (0.0, top) for q in (0.0, top)] + [(0.5, 0.5), (0.0, 0.5), (0.5, top)], np.float32)
    oc, dc = pkg.api.camera_lens_ray_host(eye, U, V, W, 8, 8, np.zeros((len(corners), 2), np.int32), np.full((len(corners), 2), 0.5, np.float32), corners, 1.0, 1.0)
    assert np.isfinite(oc).all() and np.isfinite(dc).all()
    assert ((oc.astype(np.float64) ** 2).sum(1) <= 1 + 4 * EPS).all(), (oc ** 2).sum(1)
    assert (oc[4] == 0).all()       # the centre of the square is the centre of the disc


def test_the_recount_of_a_lens_film_stays_under_its_cap(pkg, hip_lib, ob):
    """The float64 recount that tests/test_gpu_lens.py holds the "lt" film to (tests/lens_film.py), run on the ORACLE's cache of the
    Cornell box (48 x 32, 2 000 light paths, lens 3 % of |W|, focus 0.7), visibility from the oracle's own any-hit: the pixels it
    leaves out as hanging on a float32 decision stay under the cap of 3 % of the lit pixels, and it lights what a film should."""
    scene = pkg.scenes.cornell_box()
    w, h = W_, H_
    cam = scene.camera
    o = ob.Oracle(scene)
    o.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
    o.resize(w, h)
    o.set_light_trace(2000, 16, 1)
    o.set_subspace()
    o.launch("light trace", 1)
    o.build_sampler()
    v = o.lvc_read()
    _, _, _, vc, pc = o.sampler_read()
    assert vc == len(v) and pc == 2000
    _, _, _, Wv = frames(pkg)["orthogonal"]
    R = float(np.float32(0.03 * np.linalg.norm(Wv)))
    film, excluded, lit, survivors, total = host_film(pkg, ob, o, scene, v, pc, w, h, R, 0.7)
    share = (excluded & lit).sum() / max(1, lit.sum())
    print(f"oracle cache: {total} vertices, {survivors} splat; lit pixels {int(lit.sum())}, excluded {int((excluded & lit).sum())} ({share:.4f}); film mean {film.mean():.4f}")
    assert survivors > 500 and lit.sum() > 300
    assert share <= 0.03, share
    assert np.isfinite(film).all() and film.mean() > 0
    # the pinhole recount of the same cache differs: the lens moves a sizeable share of the vertices to another pixel
    sharp, _, _, _, _ = host_film(pkg, ob, o, scene, v, pc, w, h, 0.0, 0.7)
    moved = (np.abs(film - sharp).sum(-1) > 0).mean()
    print(f"pixels whose recount differs between the lens and the pinhole: {moved:.3f}")
    assert moved > 0.2 and abs(film.sum() / sharp.sum() - 1) < 0.2


def test_lens_sample_host_is_the_kernels_stream(pkg, hip_lib):
    """spcbpt_lens_sample_host against tea4 / rnd written out here: the jitter is 0.5 and draws nothing at subframe 0, the two lens
    numbers follow; a cache slot's stream has no jitter at any subframe."""
    def tea4(v0, v1):
        s0, m = 0, 0xffffffff
        for _ in range(4):
            s0 = (s0 + 0x9e3779b9) & m
            v0 = (v0 + ((((v1 << 4) & m) + 0xa341316c) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4))) & m
            v1 = (v1 + ((((v0 << 4) & m) + 0xad90777d) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761e))) & m
        return v0

    def rnd(s):
        s = (1664525 * s + 1013904223) & 0xffffffff
        return s, np.float32((s & 0x00ffffff) / float(0x01000000))

    for index, sub in ((0, 0), (17, 0), (1535, 3), (123456, 7)):
        for with_jitter in (True, False):
            s = tea4(index, sub)
            want = [np.float32(0.5), np.float32(0.5)]
            if with_jitter and sub != 0:
                s, want[0] = rnd(s)
                s, want[1] = rnd(s)
            s, u1 = rnd(s)
            s, u2 = rnd(s)
            got = pkg.api.lens_sample_host(index, sub, with_jitter)
            assert got.tobytes() == np.array(want + [u1, u2], np.float32).tobytes(), (index, sub, with_jitter, got)
    many = pkg.api.lens_sample_host(np.arange(5), 2, False)
    assert many.shape == (5, 4) and (many[:, :2] == 0.5).all() and ((many[:, 2:] >= 0) & (many[:, 2:] < 1)).all()


def test_host_forms_refuse_bad_values(pkg, hip_lib):
    eye, U, V, W = frames(pkg)["orthogonal"]
    xy, j, u = samples(np.random.default_rng(8), 4)
    for radius, focus in ((-1.0, 1.0), (0.1, 0.0), (0.1, -2.0), (float("nan"), 1.0), (0.1, float("inf"))):
        with pytest.raises(ValueError):
            pkg.api.camera_lens_ray_host(eye, U, V, W, W_, H_, xy, j, u, radius, focus)
        with pytest.raises(ValueError):
            pkg.api.camera_splat_lens(eye, U, V, W, W_, H_, np.zeros((4, 3), np.float32), u, radius, focus)
    for name in ("spcbpt_set_lens", "spcbpt_get_lens", "spcbpt_camera_lens_ray_host", "spcbpt_camera_splat_lens", "spcbpt_lens_sample_host", "spcbpt_debug_lens_rays"):
        assert name in pkg.api.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
