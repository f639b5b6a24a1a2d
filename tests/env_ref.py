"""Float64 numpy definitions of the environment map as a light and of the bilinear texture lookup, written from the definitions
(not from the device code's operation order) and shared by tests/test_gpu_env_first_principles.py, tests/test_gpu_tex_fetch.py and
tests/test_env_table_cpu.py.

  direction <-> (u, v)   u = (atan2(x, z) + pi) / 2 pi, v = (1 + y) / 2 (the device's sin(pi / 2 - acos y) IS y), y clipped to
                         [-1, 1] first.  The map is equal-area: equal (u, v) area is equal solid angle, 4 pi / size per texel.
  texture                texture row j is raster row h - 1 - j: raster row 0 (the top of the image) is the zenith (v = 1).
  bilinear lookup        texel centres at integer + 0.5: unnormalised coordinate u W - 0.5, wrap in both axes (also the lookup of the
                         RGBA8 material textures, bytes / 255).
  sampling table         over the raster AS READ (texel i = column i % W of raster row i / W is drawn for u in [i % W, i % W + 1) / W,
                         v in [i / W, i / W + 1) / H -- upstream's: the table is not flipped): v_i = the luminance r + g + b of raster
                         texel i plus the mean luminance of the cells of the diamond |dx| + |dy| <= 2 around it that lie inside the
                         image (thirteen at most: upstream's surroundsIndex keeps the texel itself in the diamond),
                         p_i = 0.75 v_i / sum(v) + 0.25 / size, pdf per solid angle p_i size / 4 pi.
  label                  NUM_SUBSPACE - 1 - (floor(u D) D + floor(v D)), both floors clamped to [0, D - 1].
  launch disk            centre c + 10 r d, radius r, normal d, uniform on the disk: density 1 / (pi r^2)."""
import numpy as np

NUM_SUBSPACE = 1000
UNIFORM_RATE = 0.25


def dir2uv(d):
    """(n, 3) directions (any length close to 1: y is clipped) -> u, v in float64."""
    d = np.asarray(d, np.float64)
    u = (np.arctan2(d[..., 0], d[..., 2]) + np.pi) / (2 * np.pi)
    v = 0.5 * (1.0 + np.clip(d[..., 1], -1.0, 1.0))
    return u, v


def uv2dir(u, v):
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    y = 2 * v - 1
    s = np.sqrt(np.maximum(0.0, 1 - y * y))
    th = 2 * np.pi * u - np.pi
    return np.stack([s * np.sin(th), y, s * np.cos(th)], -1)


def texture(raster):
    """(h, w, 4) float64 texture of an (h, w, >= 3) raster: rows flipped, alpha 1."""
    r = np.asarray(raster, np.float64)
    t = np.ones(r.shape[:2] + (4,))
    t[..., :3] = r[::-1, :, :3]
    return t


def bilinear_taps(x, y, w, h):
    """Unnormalised coordinates (texel centres at integers; float64) -> (x0, x1, y0, y1, ax, ay) with wrap."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    fx, fy = np.floor(x), np.floor(y)
    x0, y0 = np.mod(fx, w).astype(np.int64), np.mod(fy, h).astype(np.int64)
    return x0, (x0 + 1) % w, y0, (y0 + 1) % h, x - fx, y - fy


def bilinear_at(tex, x, y):
    """tex (h, w, c) looked up at unnormalised coordinates x, y (texel centres at integers)."""
    tex = np.asarray(tex, np.float64)
    h, w = tex.shape[:2]
    x0, x1, y0, y1, ax, ay = bilinear_taps(x, y, w, h)
    ax, ay = ax[..., None], ay[..., None]
    return (1 - ax) * (1 - ay) * tex[y0, x0] + ax * (1 - ay) * tex[y0, x1] + (1 - ax) * ay * tex[y1, x0] + ax * ay * tex[y1, x1]


def bilinear(tex, u, v):
    """tex (h, w, c) at normalised (u, v): the texture unit's linear filter with wrap addressing."""
    h, w = np.asarray(tex).shape[:2]
    return bilinear_at(tex, np.asarray(u, np.float64) * w - 0.5, np.asarray(v, np.float64) * h - 0.5)


def local_contrast(tex, u, v):
    """(n,) W |t10 - t00| + H |t01 - t00| (largest channel) of the bilinear cell around (u, v), and the largest of its four texels:
    the colour's sensitivity to an error in (u, v), and its scale."""
    tex = np.asarray(tex, np.float64)[..., :3]
    h, w = tex.shape[:2]
    x0, x1, y0, y1, _, _ = bilinear_taps(np.asarray(u, np.float64) * w - 0.5, np.asarray(v, np.float64) * h - 0.5, w, h)
    t00, t10, t01, t11 = tex[y0, x0], tex[y0, x1], tex[y1, x0], tex[y1, x1]
    # (the slope along x at the far row and along y at the far column count too: the cell's largest)
    gx = np.maximum(np.abs(t10 - t00), np.abs(t11 - t01)).max(-1)
    gy = np.maximum(np.abs(t01 - t00), np.abs(t11 - t10)).max(-1)
    big = np.maximum(np.maximum(np.abs(t00), np.abs(t10)), np.maximum(np.abs(t01), np.abs(t11))).max(-1)
    return w * gx + h * gy, big


def env_color(raster, d):
    u, v = dir2uv(d)
    return bilinear(texture(raster), u, v)[..., :3]


def table(raster):
    """(size,) float64 probabilities p_i of the texels of the raster as read."""
    r = np.asarray(raster, np.float64)
    h, w = r.shape[:2]
    lum = r[..., 0] + r[..., 1] + r[..., 2]
    pad = np.zeros((h + 4, w + 4))
    cnt = np.zeros((h + 4, w + 4))
    pad[2:-2, 2:-2] = lum
    cnt[2:-2, 2:-2] = 1.0
    s, n = np.zeros((h, w)), np.zeros((h, w))
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if abs(dx) + abs(dy) <= 2:
                s += pad[2 + dy:2 + dy + h, 2 + dx:2 + dx + w]
                n += cnt[2 + dy:2 + dy + h, 2 + dx:2 + dx + w]
    val = (lum + s / n).reshape(-1)
    return (1 - UNIFORM_RATE) * val / val.sum() + UNIFORM_RATE / val.size


def texel_of(u, v, w, h):
    """The table's texel index of (u, v), and the distance of u W / v H from the nearest integer (a border)."""
    x, y = np.asarray(u, np.float64) * w, np.asarray(v, np.float64) * h
    cx, cy = np.minimum(np.floor(x), w - 1).astype(np.int64), np.minimum(np.floor(y), h - 1).astype(np.int64)
    edge = np.minimum(np.abs(x - np.rint(x)), np.abs(y - np.rint(y)))
    return cx + cy * w, edge


def env_pdf(raster, d):
    """pdf per solid angle of the directions d, and their distance from a texel border (in texels)."""
    h, w = np.asarray(raster).shape[:2]
    u, v = dir2uv(d)
    i, edge = texel_of(u, v, w, h)
    return table(raster)[i] * (w * h) / (4 * np.pi), edge


def env_label(d, div_level):
    """label of the directions d, and their distance from a cell border (in cells)."""
    u, v = dir2uv(d)
    D = int(div_level)
    x, y = u * D, v * D
    ux, uy = np.clip(np.floor(x), 0, D - 1).astype(np.int64), np.clip(np.floor(y), 0, D - 1).astype(np.int64)
    edge = np.minimum(np.abs(x - np.rint(x)), np.abs(y - np.rint(y)))
    return NUM_SUBSPACE - 1 - (ux * D + uy), edge


def rgba8_texture(rgba8):
    """(h, w, 4) uint8 -> float64 in [0, 1]"""
    return np.asarray(rgba8, np.float64) / 255.0
