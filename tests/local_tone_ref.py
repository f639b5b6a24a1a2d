"""The local tone stage (include/spcbpt.h: spcbpt_local_tone) in numpy float64 with the true log2 / exp2 -- the definition
the host form and the kernels are held to -- with the bar, the seeded HDR images and three deliberately wrong variants the bar must
reject.

  1. Y = 0.3 r + 0.6 g + 0.1 b;  a pixel takes part iff 0 < Y < inf;  L = log2(min(max(Y, 2^-16), 2^16));  z = (L + 16) / rho
  2. node (gx, gy, gz), GX = (W - 1) // s + 2, GY likewise, NZ = floor(32 / rho) + 2:
       A = sum wx wy wz L,  B = sum wx wy wz  over the pixels that take part,
       wx = max(s - |x - gx s|, 0) / s,  wy likewise,  wz = max(1 - |z - gz|, 0)
  3. `blur` times: along x, then y, then z:  out(i) = 0.25 v(i - 1) + 0.5 v(i) + 0.25 v(i + 1), indices clamped
  4. ix = x // s, tx = (x - ix s) / s, the same in y, iz = min(floor(z), NZ - 2), tz = z - iz; trilinear A and B; base = A / B if B > 0 else L
  5. g = (c - 1)(base - La) + (d - 1)(L - base), La = log2(anchor), g clamped to [-32, 32];  O_rgb = I_rgb 2^g,  O_a = I_a;
     a pixel that takes no part keeps its four floats

The parameters are taken at their float32 values (the fields of spcbpt_local_tone_params) and NZ as the library computes it (the
quotient 32 / rho in float32), everything after that is float64.  Whether a pixel takes part is decided on the float32 image.

The bar between the host form and this definition, derived and not tuned.  In g:
    bar_g = (|c - 1| + |d - 1|) (2 2^-13 + (n + 8) 2^-24 16)
  * 2^-13 is the condition on lt_log2: once for the pixel's own L, once for the base, which is a weighted mean of such L;
  * a node's A is a float32 sum of at most n = (2 s - 1)^2 terms |w L| <= 16 w, so that A / B is off by at most n 2^-24 16; the 8 cover
    the roundings of the weights, the blur passes and the three lerps;
  * g is linear in base and L with the slopes (c - 1) - (d - 1) and (d - 1), which |c - 1| + |d - 1| bounds.
The output's relative bar is  ln 2 bar_g + 2^-13 + 4 2^-24:  d(2^g) / 2^g = ln 2 dg, the condition on lt_exp2, the last product."""
import numpy as np

DEFAULTS = dict(cell=16, range=1.0, blur=1, compress=0.5, detail=1.0, anchor=0.18)
# (width, height, cell, range): the smallest shapes at which each part can go wrong
SHAPES = ((1, 1, 16, 1.0),       # the minimum image
          (7, 1, 4, 1.0),        # one pixel high
          (1, 7, 4, 1.0),        # one pixel wide
          (37, 23, 8, 1.0),      # no multiple of the cell, three or more cells each way
          (5, 3, 64, 1.0),       # the image inside one cell
          (130, 70, 4, 1.0),     # many columns; crosses every block edge of the slice kernel
          (37, 23, 16, 0.5),     # NZ = 66: more bins than a wave has lanes
          (40, 40, 16, 8.0))     # NZ = 6
PARAM_SETS = (dict(),                                                      # the defaults: compress 0.5, detail 1, blur 1
              dict(compress=0.3, detail=1.5, blur=0, anchor=1.0),
              dict(compress=1.5, detail=0.5, blur=4, anchor=0.05))
MUTANTS = ("flat_wz", "swap_txy", "no_division")


def shape_id(shape):
    w, h, s, rho = shape
    return f"{w}x{h}-s{s}-r{rho:g}"


def plan(width, height, cell, rho):
    """(GX, GY, NZ) as local_tone_plan_of computes them."""
    return (width - 1) // cell + 2, (height - 1) // cell + 2, int(np.float32(32.0) / np.float32(rho)) + 2


def takes_part(img):
    """(h, w) bool, on the float32 image in the library's order of operations."""
    x = np.asarray(img, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        Y = (np.float32(0.3) * x[..., 0] + np.float32(0.6) * x[..., 1]) + np.float32(0.1) * x[..., 2]
        return (Y > 0) & (Y < np.inf)


def _blur_axis(v, axis):
    n = v.shape[axis]
    i = np.arange(n)
    lo, hi = np.take(v, np.clip(i - 1, 0, n - 1), axis), np.take(v, np.clip(i + 1, 0, n - 1), axis)
    return 0.25 * lo + 0.5 * v + 0.25 * hi


def local_tone(img, mutant=None, absent=None, **params):
    """The (h, w, 4) image through the stage.  `absent`: an (h, w) bool mask of pixels to leave out of the grid as if they took no part
    (they still get an output when they take part).  Returns dict(O (h, w, 4), part, L, base, g (h, w))."""
    p = dict(DEFAULTS, **params)
    s, nblur = int(p["cell"]), int(p["blur"])
    rho, c, d, anchor = (np.float64(np.float32(p[k])) for k in ("range", "compress", "detail", "anchor"))
    I = np.asarray(img, dtype=np.float32).astype(np.float64)
    H, W = I.shape[:2]
    GX, GY, NZ = plan(W, H, s, rho)
    part = takes_part(img)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        Y = 0.3 * I[..., 0] + 0.6 * I[..., 1] + 0.1 * I[..., 2]
        L = np.where(part, np.log2(np.clip(np.where(part, Y, 1.0), 2.0 ** -16, 2.0 ** 16)), 0.0)
    z = (L + 16.0) / rho
    # 2. the gather, as dense tent matrices
    in_grid = part if absent is None else part & ~absent
    WX = np.maximum(s - np.abs(np.arange(W)[None, :] - s * np.arange(GX)[:, None]), 0) / s          # GX, W
    WY = np.maximum(s - np.abs(np.arange(H)[None, :] - s * np.arange(GY)[:, None]), 0) / s          # GY, H
    WZ = np.maximum(1.0 - np.abs(z[..., None] - np.arange(NZ)[None, None, :]), 0.0)                 # H, W, NZ
    if mutant == "flat_wz":
        WZ = np.ones_like(WZ)
    WZ = WZ * in_grid[..., None]
    A = np.einsum("gy,yhz->ghz", WY, np.einsum("hx,yxz->yhz", WX, WZ * L[..., None]))               # GY, GX, NZ
    B = np.einsum("gy,yhz->ghz", WY, np.einsum("hx,yxz->yhz", WX, WZ))
    # 3. blur
    for _ in range(nblur):
        for axis in (1, 0, 2):      # x, then y, then z
            A, B = _blur_axis(A, axis), _blur_axis(B, axis)
    # 4. slice
    ys, xs = np.mgrid[0:H, 0:W]
    ix, iy = xs // s, ys // s
    tx, ty = (xs - ix * s) / s, (ys - iy * s) / s
    if mutant == "swap_txy":
        tx, ty = ty, tx
    iz = np.minimum(np.floor(z).astype(np.int64), NZ - 2)
    iz = np.where(part, iz, 0)
    tz = z - iz

    def tri(G):
        def col(gy, gx):
            return G[gy, gx, iz] + tz * (G[gy, gx, iz + 1] - G[gy, gx, iz])
        r0 = col(iy, ix) + tx * (col(iy, ix + 1) - col(iy, ix))
        r1 = col(iy + 1, ix) + tx * (col(iy + 1, ix + 1) - col(iy + 1, ix))
        return r0 + ty * (r1 - r0)
    a, b = tri(A), tri(B)
    with np.errstate(invalid="ignore", divide="ignore"):
        base = np.where(b > 0, a / np.where(b > 0, b, 1.0), L)
    if mutant == "no_division":
        base = a
    # 5. gain
    La = np.log2(anchor)
    g = np.clip((c - 1.0) * (base - La) + (d - 1.0) * (L - base), -32.0, 32.0)
    O = I.copy()
    k = np.where(part, 2.0 ** g, 1.0)
    with np.errstate(invalid="ignore"):
        O[..., :3] = np.where(part[..., None], I[..., :3] * k[..., None], I[..., :3])
    return dict(O=O, part=part, L=L, base=base, g=g, b=b)


def bar_g(cell, compress, detail):
    n = (2 * cell - 1) ** 2
    c, d = np.float64(np.float32(compress)), np.float64(np.float32(detail))
    return (abs(c - 1.0) + abs(d - 1.0)) * (2.0 * 2.0 ** -13 + (n + 8) * 2.0 ** -24 * 16.0)


def bar_rel(cell, compress, detail):
    """The relative bar of an output channel of a pixel that takes part."""
    return np.log(2.0) * bar_g(cell, compress, detail) + 2.0 ** -13 + 4 * 2.0 ** -24


def excess(out, r, **params):
    """max over the channels of the pixels that take part of |out - O_ref| / (bar |O_ref|) (<= 1 passes), and their number."""
    p = dict(DEFAULTS, **params)
    part = r["part"]
    ref = r["O"][..., :3][part]
    err = np.abs(np.asarray(out, dtype=np.float64)[..., :3][part] - ref)
    bound = bar_rel(p["cell"], p["compress"], p["detail"]) * np.abs(ref) + 1e-300
    return (float((err / bound).max()) if err.size else 0.0), int(part.sum())


# ------------------------------------------------------------------------------------------------------------ images
def seeded_image(width, height, seed=0):
    """Luminance 2^U(-10, 10), a random chroma in [0.2, 1] per channel, alpha U(0, 1): twenty stops, neighbours far apart."""
    rng = np.random.default_rng(9000 * width + height + seed)
    img = np.empty((height, width, 4), np.float32)
    img[..., :3] = (2.0 ** rng.uniform(-10.0, 10.0, (height, width, 1)) * rng.uniform(0.2, 1.0, (height, width, 3))).astype(np.float32)
    img[..., 3] = rng.uniform(0.0, 1.0, (height, width)).astype(np.float32)
    return img


def planted_image(width, height, seed=0):
    """seeded_image with pixels that take no part at known places: a NaN channel, a +inf channel, a -inf channel, an all-zero pixel, a
    negative pixel, and one pixel below 2^-16 and one above 2^16, which take part at the clamped luminance.  Returns (image, plants)
    with plants = {"nan" | "pinf" | "ninf" | "zero" | "negative" | "tiny" | "huge": [(y, x)]}.  An image of fewer than eight pixels
    carries what fits: a NaN in its first pixel and a zero pixel in its last if it has more than one."""
    img = seeded_image(width, height, seed)
    n = width * height
    plants = {k: [] for k in ("nan", "pinf", "ninf", "zero", "negative", "tiny", "huge")}

    def put(kind, i, rgb):
        y, x = divmod(i % n, width)
        for ch, v in enumerate(rgb):
            if v is not None:
                img[y, x, ch] = v
        plants[kind].append((y, x))
    if n < 8:
        if n > 1:
            put("nan", 0, (None, np.nan, None))
            put("zero", n - 1, (0.0, 0.0, 0.0))
        return img, plants
    at = [(k * n) // 7 + (1 if k else 0) for k in range(7)]
    put("nan", at[0], (None, np.nan, None))
    put("pinf", at[1], (None, None, np.inf))
    put("ninf", at[2], (-np.inf, None, None))
    put("zero", at[3], (0.0, 0.0, 0.0))
    put("negative", at[4], (-1.0, -2.0, -0.5))
    put("tiny", at[5], (1e-7, 2e-7, 1e-7))
    put("huge", at[6], (3.0e5, 2.0e5, 1.0e5))
    assert len({v for k in plants.values() for v in k}) == 7
    return img, plants


def no_part_mask(plants, shape):
    m = np.zeros(shape, bool)
    for kind in ("nan", "pinf", "ninf", "zero", "negative"):
        for (y, x) in plants[kind]:
            m[y, x] = True
    return m


def edge_image(width=23, height=37, left=-4.0, right=8.0):
    """A grey image, the columns left of the middle at log-luminance `left`, the others at `right`."""
    img = np.ones((height, width, 4), np.float32)
    img[:, : width // 2, :3] = np.float32(2.0 ** left)
    img[:, width // 2:, :3] = np.float32(2.0 ** right)
    return img
