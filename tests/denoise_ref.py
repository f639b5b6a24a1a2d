"""Float64 numpy recomputation of the a-trous denoiser of include/spcbpt.h (spcbpt_denoise / spcbpt_denoise_host), written from the
formula in the header and shared by tests/test_denoise_host.py and tests/test_gpu_denoise.py, plus the film's tone map."""
import numpy as np

KERNEL = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
ALBEDO_FLOOR = 1e-3


def pixel_centre_dirs(U, V, W, width, height):
    """(h, w, 3) float64: the normalised direction through the centre of every pixel (camera_ray with jitter 0.5)."""
    U, V, W = (np.asarray(v, dtype=np.float64) for v in (U, V, W))
    dx = 2.0 * ((np.arange(width) + 0.5) / width) - 1.0
    dy = 2.0 * ((np.arange(height) + 0.5) / height) - 1.0
    d = dx[None, :, None] * U + dy[:, None, None] * V + W
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def atrous_ref(accum, albedo, normal_depth, U, V, W, iterations, sigma_c, sigma_n, sigma_x):
    """denoised rgb, (h, w, 3) float64, from (h, w, 4) inputs."""
    h, w = accum.shape[:2]
    alb = np.maximum(albedo[..., :3].astype(np.float64), ALBEDO_FLOOR)
    c = accum[..., :3].astype(np.float64) / alb
    n = normal_depth[..., :3].astype(np.float64)
    X = pixel_centre_dirs(U, V, W, w, h) * normal_depth[..., 3:4].astype(np.float64)
    for i in range(iterations):
        s = 1 << i
        L = 0.3 * c[..., 0] + 0.6 * c[..., 1] + 0.1 * c[..., 2]
        num, den = np.zeros_like(c), np.zeros((h, w))
        for b in range(-2, 3):
            for a in range(-2, 3):
                oy, ox = s * b, s * a
                y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
                if y0 >= y1 or x0 >= x1:
                    continue   # every tap of this offset lies outside the image
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                e = (-((c[Q] - c[P]) ** 2).sum(-1) / ((sigma_c * 2.0 ** -i) ** 2 * (1e-2 + (L[P] + L[Q]) / 2) ** 2)
                     - ((n[Q] - n[P]) ** 2).sum(-1) / sigma_n ** 2
                     - ((X[Q] - X[P]) ** 2).sum(-1) / (sigma_x * s) ** 2)
                wgt = KERNEL[a + 2] * KERNEL[b + 2] * np.exp(e)
                num[P] += wgt[..., None] * c[Q]
                den[P] += wgt
        c = num / den[..., None]
    return c * alb


def tone_map_codes(rgb):
    """film_write's tone map of (h, w, 3) radiance in float64, as UNROUNDED codes x * 256 (floor + clamp to 255 gives the byte)."""
    rgb = np.asarray(rgb, dtype=np.float64)
    lum = 0.3 * rgb[..., 0] + 0.6 * rgb[..., 1] + 0.1 * rgb[..., 2]
    t = np.clip(rgb / (1.0 + lum / 1.5)[..., None], 0.0, 1.0)
    srgb = np.where(t < 0.0031308, 12.92 * t, 1.055 * np.power(t, 1 / 2.4) - 0.055)
    return np.clip(srgb, 0.0, 1.0) * 256.0
