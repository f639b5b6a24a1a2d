"""Numpy restatement of the history reprojection of include/spcbpt.h (spcbpt_history_reproject / spcbpt_history_resolve), written from
the formula in the header, float64 by default with the dtype selectable (float32 shows what rounding alone does to the formula).
Shared by tests/test_reproject_host.py and tests/test_gpu_reproject.py."""
import numpy as np


def lookat_camera(eye, lookat, up, fov, aspect):
    """(eye, U, V, W) float32 as spcbpt_set_camera_lookat builds them, computed in float64."""
    eye, lookat, up = (np.asarray(v, np.float64) for v in (eye, lookat, up))
    W = lookat - eye
    U = np.cross(W, up)
    U /= np.linalg.norm(U)
    V = np.cross(U, W)
    V /= np.linalg.norm(V)
    V *= np.linalg.norm(W) * np.tan(0.5 * np.radians(fov))
    U *= np.linalg.norm(V) * aspect
    return tuple(np.asarray(v, np.float32) for v in (eye, U, V, W))


def centre_rays(U, V, W, width, height, dtype=np.float64):
    """(h, w, 3): the UNNORMALISED direction dx U + dy V + W through the centre of every pixel (camera_ray with jitter 0.5)."""
    T = np.dtype(dtype).type
    U, V, W = (np.asarray(v, dtype) for v in (U, V, W))
    dx = T(2) * ((np.arange(width, dtype=dtype) + T(0.5)) / T(width)) - T(1)
    dy = T(2) * ((np.arange(height, dtype=dtype) + T(0.5)) / T(height)) - T(1)
    return dx[None, :, None] * U + dy[:, None, None] * V + W


def positions(cam, normal_depth, dtype=np.float64):
    """(h, w, 3): eye + d_c depth, the first hit of every pixel's centre ray."""
    eye, U, V, W = (np.asarray(v, dtype) for v in cam)
    nd = np.asarray(normal_depth, dtype)
    h, w = nd.shape[:2]
    d = centre_rays(U, V, W, w, h, dtype)
    d = d / np.sqrt((d * d).sum(-1, keepdims=True))
    return eye + d * nd[..., 3:4]


def project(cam_h, P, dtype=np.float64):
    """(g, dx, dy) of world points P in the camera cam_h: the algebra of camera_splat."""
    eye, U, V, W = (np.asarray(v, dtype) for v in cam_h)
    c = np.asarray(P, dtype) - eye
    D = U @ np.cross(V, W)
    with np.errstate(all="ignore"):
        g = (c @ np.cross(U, V)) / D
        dx = ((c @ np.cross(V, W)) / D) / g
        dy = ((c @ np.cross(W, U)) / D) / g
    return g, dx, dy


def tap_coordinates(d, size, dtype=np.float64):
    T = np.dtype(dtype).type
    f = np.clip((d + T(1)) * T(0.5) * T(size) - T(0.5), T(-2), T(size + 1))
    f = np.where(np.isnan(f), T(-2), f)
    f0 = np.floor(f)
    return f0.astype(np.int64), (f - f0).astype(dtype)


def reproject_ref(cam, normal_depth, cam_h, G, H, sigma_n, sigma_x, max_history, dtype=np.float64, details=False):
    """The prior R, (h, w, 4) of `dtype`, from the current features, the history camera and the history planes G = (normal, depth),
    H = (rgb, n).  With details=True also a dict: S, the live mask (a hit with g > 0), x0, y0, ax, ay, P."""
    T = np.dtype(dtype).type
    nd, G, H = (np.asarray(a, dtype) for a in (normal_depth, G, H))
    h, w = nd.shape[:2]
    P = positions(cam, nd, dtype)
    g, dx, dy = project(cam_h, P, dtype)
    live = (nd[..., 3] > 0) & (g > 0)
    x0, ax = tap_coordinates(np.where(live, dx, T(-9)), w, dtype)
    y0, ay = tap_coordinates(np.where(live, dy, T(-9)), h, dtype)
    Xh = positions(cam_h, G, dtype)
    n = nd[..., :3]
    S, C, N = np.zeros((h, w), dtype), np.zeros((h, w, 3), dtype), np.zeros((h, w), dtype)
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = x0 + i, y0 + j
            inside = live & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            qxc, qyc = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            Gq, Hq, Xq = G[qyc, qxc], H[qyc, qxc], Xh[qyc, qxc]
            ok = inside & (Gq[..., 3] > 0)
            b = (ax if i else T(1) - ax) * (ay if j else T(1) - ay)
            plane = (n * (Xq - P)).sum(-1)
            e = -(plane * plane) / T(sigma_x) ** 2 - ((Gq[..., :3] - n) ** 2).sum(-1) / T(sigma_n) ** 2
            wq = np.where(ok, b * np.exp(e), T(0)).astype(dtype)
            S += wq
            C += wq[..., None] * Hq[..., :3]
            N += wq * Hq[..., 3]
    R = np.zeros((h, w, 4), dtype)
    keep = S >= T(1e-6)
    Ss = np.where(keep, S, T(1))
    R[..., :3] = np.where(keep[..., None], C / Ss[..., None], T(0))
    R[..., 3] = np.where(keep, Ss * np.minimum(N / Ss, T(max_history)), T(0))
    if details:
        return R, dict(S=S, live=live, x0=x0, y0=y0, ax=ax, ay=ay, P=P)
    return R


def resolve_ref(prior, accum, frames, dtype=np.float64):
    """out = ((m R.rgb + Nf accum.rgb) / (m + Nf), m + Nf), m = R.w (0 without a prior)."""
    a = np.asarray(accum, dtype)
    r = np.zeros_like(a) if prior is None else np.asarray(prior, dtype)
    nf = np.dtype(dtype).type(frames)
    m = r[..., 3:4]
    out = np.empty_like(a)
    out[..., :3] = (m * r[..., :3] + nf * a[..., :3]) / (m + nf)
    out[..., 3] = m[..., 0] + nf
    return out


def orbit(eye, lookat, degrees, distance=None, y=None):
    """The eye turned by `degrees` about the vertical axis through the look-at point, optionally put `distance` away from it
    (horizontally measured) and raised to height y."""
    eye, lookat = np.asarray(eye, np.float64), np.asarray(lookat, np.float64)
    d = eye - lookat
    a = np.radians(degrees)
    r = np.array([d[0] * np.cos(a) + d[2] * np.sin(a), d[1], -d[0] * np.sin(a) + d[2] * np.cos(a)])
    if distance is not None:
        r[[0, 2]] *= distance / np.hypot(r[0], r[2])
    out = lookat + r
    if y is not None:
        out[1] = y
    return out
