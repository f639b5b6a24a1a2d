"""The bloom stage (include/spcbpt.h: spcbpt_bloom) in numpy float64 -- the definition the host form and the kernels are
held to -- with the bar, the seeded HDR images and three deliberately wrong variants the bar must reject.

  1. C = I > 0 ? min(I, K) : 0;  Y = 0.3 Cr + 0.6 Cg + 0.1 Cb;  t = Y > T ? (Y - T) / Y : 0;  P = C t
  2. D_0 = P;  D_{k+1}(x, y) = sum_j sum_i w_j w_i D_k(cx(2x - 1 + i), cy(2y - 1 + j)),  w = (1, 3, 3, 1) / 8,  size ceil(./2)
  3. g_k = q^(k-1) / sum_m q^(m-1);  U_L = g_L D_L;  U_k = g_k D_k + up(U_{k+1});  B = up(U_1)
  4. O = I + s (B - P),  alpha copied

The parameters are taken at their float32 values (the fields of spcbpt_bloom_params), everything after that is float64."""
import numpy as np

DEFAULTS = dict(levels=5, strength=0.1, spread=1.0, threshold=0.0, clamp=65504.0)
W4 = np.array([1.0, 3.0, 3.0, 1.0]) / 8.0
SIZES = ((1, 1), (9, 1), (7, 5), (43, 29), (130, 67))   # (width, height)
LEVELS = (1, 3, 8)
SPREADS = (0.5, 1.0, 2.0)
THRESHOLDS = (0.0, 1.0)
MUTANTS = ("zero_pad", "swap_up", "drop_coarsest")


def _taps(n_out, n_in, zero_pad):
    """(n_out, 4) source indices 2x - 1 + i clamped to the edge, and a (n_out, 4) mask of the taps that fell outside (used by the
    zero-padding mutant only)."""
    raw = 2 * np.arange(n_out)[:, None] - 1 + np.arange(4)[None, :]
    inside = (raw >= 0) & (raw <= n_in - 1)
    return np.clip(raw, 0, n_in - 1), (inside if zero_pad else np.ones_like(inside))


def down(A, zero_pad=False):
    H, W = A.shape[:2]
    h, w = (H + 1) // 2, (W + 1) // 2
    xs, mx = _taps(w, W, zero_pad)
    ys, my = _taps(h, H, zero_pad)
    rows = (A[:, xs] * (W4 * mx)[None, :, :, None]).sum(2)          # H, w, 3: the horizontal sums first
    return (rows[ys] * (W4 * my)[:, :, None, None]).sum(1)           # h, w, 3


def up(A, H, W, swap=False):
    h, w = A.shape[:2]
    near, far = (0.25, 0.75) if swap else (0.75, 0.25)

    def idx(n, m):
        x = np.arange(n)
        p = x >> 1
        return p, np.clip(p + np.where(x & 1, 1, -1), 0, m - 1)
    py, ny = idx(H, h)
    px, nx = idx(W, w)
    rows = near * A[:, px] + far * A[:, nx]
    return near * rows[py] + far * rows[ny]


def clipped(I, K):
    with np.errstate(invalid="ignore"):
        return np.where(I > 0, np.minimum(I, K), 0.0)


def blur(P, levels, spread, mutant=None):
    """B = up(U_1) of steps 2 and 3 for a non-negative (h, w, 3) float64 image."""
    D = [P]
    for _ in range(levels):
        D.append(down(D[-1], zero_pad=mutant == "zero_pad"))
    g = spread ** np.arange(levels)
    g = g / g.sum()
    U = g[-1] * D[levels]
    if mutant == "drop_coarsest":
        U = np.zeros_like(U)
    for k in range(levels - 1, 0, -1):
        U = g[k - 1] * D[k] + up(U, *D[k].shape[:2], swap=mutant == "swap_up")
    return up(U, *P.shape[:2], swap=mutant == "swap_up")


def bloom(img, mutant=None, **params):
    """The (h, w, 4) image through the stage.  Returns dict(O (h, w, 4), B, P, C, B0 (h, w, 3)): B0 is the blur of C, the same run with
    threshold 0, which the bar is written in."""
    p = dict(DEFAULTS, **params)
    L = int(p["levels"])
    s, q, T, K = (np.float64(np.float32(p[k])) for k in ("strength", "spread", "threshold", "clamp"))
    I = np.asarray(img, dtype=np.float32).astype(np.float64)
    rgb = I[..., :3]
    C = clipped(rgb, K)
    Y = 0.3 * C[..., 0] + 0.6 * C[..., 1] + 0.1 * C[..., 2]
    t = np.where(Y > T, (Y - T) / np.where(Y > 0, Y, 1.0), 0.0)
    P = C * t[..., None]
    B = blur(P, L, q, mutant)
    B0 = B if T == 0 and mutant is None else blur(C, L, q)
    O = I.copy()
    with np.errstate(invalid="ignore"):
        O[..., :3] = rgb + s * (B - P)
    return dict(O=O, B=B, P=P, C=C, B0=B0)


def bound(img, r, levels, strength):
    """The per-channel bar (h, w, 3):  (32 L + 16) 2^-24 (|I| + s (B0 + C)) + 1e-30.  Meaningful at the finite channels."""
    I = np.abs(np.asarray(img, dtype=np.float64)[..., :3])
    s = np.float64(np.float32(strength))
    with np.errstate(invalid="ignore"):
        return (32 * levels + 16) * 2.0 ** -24 * (I + s * (r["B0"] + r["C"])) + 1e-30


def excess(out, img, r, levels, strength):
    """max over the finite channels of |out - O_ref| / bar (<= 1 passes), and the number of finite channels."""
    finite = np.isfinite(np.asarray(img)[..., :3])
    with np.errstate(invalid="ignore"):
        err = np.abs(np.asarray(out, dtype=np.float64)[..., :3] - r["O"][..., :3])
    ratio = err[finite] / bound(img, r, levels, strength)[finite]
    return (float(ratio.max()) if ratio.size else 0.0), int(finite.sum())


# ------------------------------------------------------------------------------------------------------------ images
def seeded_image(width, height, seed=0):
    """2^U(-10, 12) per channel, float32, alpha U(0, 1): twenty-two octaves, small bright values among dark ones."""
    rng = np.random.default_rng(7000 * width + height + seed)
    img = np.empty((height, width, 4), np.float32)
    img[..., :3] = (2.0 ** rng.uniform(-10.0, 12.0, (height, width, 3))).astype(np.float32)
    img[..., 3] = rng.uniform(0.0, 1.0, (height, width)).astype(np.float32)
    return img


def planted_image(width, height, seed=0):
    """seeded_image with a handful of channels replaced at known places: negative, NaN, +inf and above the default clamp (3e5 > 65504).
    Returns (image, plants) with plants = {"negative" | "nan" | "inf" | "above": [(y, x, c), ...]}.  An image of fewer than eight
    pixels carries what fits: a NaN and a negative channel in its first pixel, an above-clamp channel in its last; +inf needs a
    pixel of its own beside finite neighbours and is left out there."""
    img = seeded_image(width, height, seed)
    n = width * height
    plants = {"negative": [], "nan": [], "inf": [], "above": []}

    def put(kind, i, c, v):
        y, x = divmod(i % n, width)
        img[y, x, c] = v
        plants[kind].append((y, x, c))
    if n < 8:
        put("nan", 0, 1, np.nan)
        put("negative", 0, 2, -3.0)
        if n > 1:
            put("above", n - 1, 0, 3.0e5)
        return img, plants
    at = [(k * n) // 7 for k in range(7)]            # seven different pixels for n >= 7, spread over the image
    put("negative", at[0], 0, -2.5)
    put("nan", at[1], 1, np.nan)
    put("above", at[2], 1, 3.0e5)
    put("inf", at[3], 2, np.inf)
    put("negative", at[4], 2, -1.0e3)
    put("above", at[5], 0, 7.0e4)
    put("nan", at[6], 0, np.nan)
    assert len({(y, x) for v in plants.values() for (y, x, _) in v}) == 7   # seven different pixels
    return img, plants


def impulse_image(width=64, height=96):
    """Two impulses at the centre of a black image: what the energy statement is made on."""
    img = np.zeros((height, width, 4), np.float32)
    img[..., 3] = 1.0
    img[height // 2, width // 2, :3] = (100.0, 50.0, 10.0)
    img[height // 2 - 3, width // 2 + 2, :3] = (3.0, 3.0, 3.0)
    return img
