"""Float64 numpy recomputations of the film's second moment, the film error and the variance-guided a-trous denoiser of
include/spcbpt.h (spcbpt_set_film_moments / spcbpt_film_error / spcbpt_denoise_variance and their _host forms), written from the
formulas in the header and shared by tests/test_film_moments_host.py and tests/test_gpu_film_moments.py."""
import numpy as np

from tests.denoise_ref import ALBEDO_FLOOR, KERNEL, pixel_centre_dirs

PRE = (1 / 4, 1 / 2, 1 / 4)
LUM = np.array([0.3, 0.6, 0.1])


def welford_ref(samples):
    """(mean, M2, n) in float64 after the frames samples[0], samples[1], ... ((frames, ..., 3)), by Welford's update."""
    xs = np.asarray(samples, dtype=np.float64)
    mean, m2 = np.zeros(xs.shape[1:]), np.zeros(xs.shape[1:])
    for f, x in enumerate(xs):
        d = x - mean
        mean = mean + d / (f + 1)
        m2 = m2 + d * (x - mean)
    return mean, m2, len(xs)


def sd_ref(m2n):
    """sd_k = sqrt(max(M2_k, 0) / (n (n - 1))) where n >= 2, else 0: (..., 3) float64."""
    m = np.asarray(m2n, dtype=np.float64)
    n = m[..., 3]
    ok = n >= 2
    nn = np.where(ok, n * (n - 1), 1.0)
    return np.where(ok[..., None], np.sqrt(np.maximum(m[..., :3], 0.0) / nn[..., None]), 0.0)


def film_error_ref(accum, m2n):
    """(pixels, mean, max) of e = (0.3 sd_r + 0.6 sd_g + 0.1 sd_b) / (1e-2 + L(accum)) over the pixels with n >= 2."""
    a = np.asarray(accum, dtype=np.float64)
    ok = np.asarray(m2n)[..., 3] >= 2
    e = (sd_ref(m2n) @ LUM) / (1e-2 + a[..., :3] @ LUM)
    if not ok.any():
        return 0, 0.0, 0.0
    return int(ok.sum()), float(e[ok].mean()), float(e[ok].max())


def _shift(h, w, oy, ox):
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 >= y1 or x0 >= x1:
        return None   # every tap of this offset lies outside the image
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def atrous_var_ref(accum, m2n, albedo, normal_depth, U, V, W, iterations, sigma_v, sigma_n, sigma_x):
    """denoised rgb, (h, w, 3) float64, from (h, w, 4) inputs."""
    h, w = accum.shape[:2]
    alb = np.maximum(albedo[..., :3].astype(np.float64), ALBEDO_FLOOR)
    c = accum[..., :3].astype(np.float64) / alb
    v = np.where(np.asarray(m2n)[..., 3] >= 2, ((sd_ref(m2n) / alb) @ LUM) ** 2, (c @ LUM) ** 2)
    n = normal_depth[..., :3].astype(np.float64)
    X = pixel_centre_dirs(U, V, W, w, h) * normal_depth[..., 3:4].astype(np.float64)
    for i in range(iterations):
        s = 1 << i
        vt, g = np.zeros((h, w)), np.zeros((h, w))
        for b in (-1, 0, 1):
            for a in (-1, 0, 1):
                P, Q = _shift(h, w, b, a)
                vt[P] += PRE[a + 1] * PRE[b + 1] * v[Q]
                g[P] += PRE[a + 1] * PRE[b + 1]
        vt /= g
        L = c @ LUM
        den_c = sigma_v ** 2 * vt + (1e-3 * (1e-2 + L)) ** 2
        num, den, vnum = np.zeros_like(c), np.zeros((h, w)), np.zeros((h, w))
        for b in range(-2, 3):
            for a in range(-2, 3):
                r = _shift(h, w, s * b, s * a)
                if r is None:
                    continue
                P, Q = r
                e = (-(L[Q] - L[P]) ** 2 / den_c[P]
                     - ((n[Q] - n[P]) ** 2).sum(-1) / sigma_n ** 2
                     - ((X[Q] - X[P]) ** 2).sum(-1) / (sigma_x * s) ** 2)
                wgt = KERNEL[a + 2] * KERNEL[b + 2] * np.exp(e)
                num[P] += wgt[..., None] * c[Q]
                den[P] += wgt
                vnum[P] += wgt ** 2 * v[Q]
        c = num / den[..., None]
        v = vnum / den ** 2
    return c * alb
