"""The thin-lens camera in float64 numpy, written from its definition, not from csrc/camera_lens.h.

Camera eye, U, V, W with D = U . (V x W) != 0; lens radius R >= 0 and focus depth f > 0 (in units of W).
  eye side   pixel sample (x + jx, y + jy): dx = 2 (x + jx) / w - 1, dy likewise; focus point F = eye + f (dx U + dy V + W);
             lens point O = eye + R (a U / |U| + b V / |V|), (a, b) the concentric map of (u1, u2); ray (O, normalize(F - O)).
  light side point P seen from O: rejected when (P - O) . (U x V) / D <= 0; F = where the line O -> P meets the plane g = f; the pixel is
             that of (dx, dy) of F; q = F - O; We = w h |q|^3 / (4 f^2 |q . (U x V)|), the reciprocal solid angle, seen from O, of the
             pixel's footprint on the plane in focus.
Everything is vectorised over the leading axis."""
import numpy as np


def disc(u1, u2):
    """Shirley-Chiu concentric map of [0, 1)^2 onto the unit disc -> (a, b)."""
    u1, u2 = np.asarray(u1, np.float64), np.asarray(u2, np.float64)
    sx, sy = 2 * u1 - 1, 2 * u2 - 1
    wide = np.abs(sx) > np.abs(sy)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(wide, sx, sy)
        phi = np.where(wide, np.pi / 4 * (sy / sx), np.pi / 2 - np.pi / 4 * (sx / sy))
    zero = (sx == 0) & (sy == 0)
    phi = np.where(zero, 0.0, phi)
    r = np.where(zero, 0.0, r)
    return r * np.cos(phi), r * np.sin(phi)


def lens_point(eye, U, V, u1, u2, radius):
    eye, U, V = (np.asarray(v, np.float64) for v in (eye, U, V))
    a, b = disc(u1, u2)
    return eye + radius * (a[..., None] * (U / np.linalg.norm(U)) + b[..., None] * (V / np.linalg.norm(V)))


def lens_ray(eye, U, V, W, w, h, x, y, jx, jy, u1, u2, radius, focus):
    """-> (origin (n, 3), direction (n, 3), dx (n,), dy (n,))."""
    eye, U, V, W = (np.asarray(v, np.float64) for v in (eye, U, V, W))
    dx = 2 * (np.asarray(x, np.float64) + np.asarray(jx, np.float64)) / w - 1
    dy = 2 * (np.asarray(y, np.float64) + np.asarray(jy, np.float64)) / h - 1
    F = eye + focus * (dx[..., None] * U + dy[..., None] * V + W)
    O = lens_point(eye, U, V, u1, u2, radius)
    d = F - O
    return O, d / np.linalg.norm(d, axis=-1, keepdims=True), dx, dy


def project(eye, U, V, W, P):
    """camera_project in float64: (g, dx, dy) of points P as seen from `eye`."""
    eye, U, V, W = (np.asarray(v, np.float64) for v in (eye, U, V, W))
    c = np.asarray(P, np.float64) - eye
    D = U @ np.cross(V, W)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = c @ np.cross(U, V) / D
        dx = (c @ np.cross(V, W) / D) / g
        dy = (c @ np.cross(W, U) / D) / g
    return g, dx, dy


def splat_lens(eye, U, V, W, w, h, P, u1, u2, radius, focus, pinhole_weight=False):
    """-> dict(inside, dx, dy, fx, fy (continuous pixel coordinates), px, py, weight, origin, g).  pinhole_weight=True is the seeded
    corruption of the Jacobian test: camera_splat's w h |c / g|^3 / (4 |D|) with c = P - eye, which ignores the lens."""
    eye, U, V, W = (np.asarray(v, np.float64) for v in (eye, U, V, W))
    P = np.asarray(P, np.float64)
    O = lens_point(eye, U, V, u1, u2, radius)
    uv = np.cross(U, V)
    D = U @ np.cross(V, W)
    c = P - O
    with np.errstate(divide="ignore", invalid="ignore"):
        g = (c @ uv) / D
        q = c * (focus / g)[..., None]
        F = O + q
        _, dx, dy = project(eye, U, V, W, F)
        weight = w * h * np.linalg.norm(q, axis=-1) ** 3 / (4 * focus * focus * np.abs(q @ uv))
        if pinhole_weight:
            ce = P - eye
            ge = (ce @ uv) / D
            weight = w * h * np.linalg.norm(ce / ge[..., None], axis=-1) ** 3 / (4 * abs(D))
    fx, fy = (dx + 1) / 2 * w, (dy + 1) / 2 * h
    inside = (g > 0) & (np.abs(dx) < 1) & (np.abs(dy) < 1)
    px = np.clip(np.floor(np.where(inside, fx, 0)), 0, w - 1).astype(int)
    py = np.clip(np.floor(np.where(inside, fy, 0)), 0, h - 1).astype(int)
    return dict(inside=inside, dx=dx, dy=dy, fx=fx, fy=fy, px=px, py=py, weight=weight, origin=O, g=g)


def footprint_solid_angle(eye, U, V, W, w, h, px, py, O, focus, n=8):
    """The solid angle, seen from O, of pixel (px, py)'s footprint on the plane g = focus: the parallelogram split into 2 n^2 triangles,
    each by Van Oosterom & Strackee's formula -- exact for a planar triangle, so n only guards the arctangent's conditioning."""
    eye, U, V, W, O = (np.asarray(v, np.float64) for v in (eye, U, V, W, O))
    total = 0.0

    def corner(i, j):
        dx = 2 * (px + i / n) / w - 1
        dy = 2 * (py + j / n) / h - 1
        return eye + focus * (dx * U + dy * V + W) - O

    def tri(a, b, c):
        la, lb, lc = np.linalg.norm(a), np.linalg.norm(b), np.linalg.norm(c)
        num = a @ np.cross(b, c)
        den = la * lb * lc + (a @ b) * lc + (a @ c) * lb + (b @ c) * la
        return abs(2 * np.arctan2(num, den))

    for i in range(n):
        for j in range(n):
            p00, p10, p01, p11 = corner(i, j), corner(i + 1, j), corner(i, j + 1), corner(i + 1, j + 1)
            total += tri(p00, p10, p11) + tri(p00, p11, p01)
    return total
