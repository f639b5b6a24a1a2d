"""The display transform (include/spcbpt.h: spcbpt_display, csrc/display_pixel.h) in numpy, written from the header text: the luminance
histogram by bit pattern, the auto EV in float64, the four tone operators in float64 as UNROUNDED codes (floor + clamp to 255 gives the
byte, as denoise_ref.tone_map_codes does for the film's curve).  Shared by test_display_host.py and test_gpu_display.py, with the
images and the byte rule both use.

The luminance that is binned is the float32 one -- the bins are cut from its bit pattern --, so it is formed in float32 in the
header's order, (0.3 r + 0.6 g) + 0.1 b; everything after the counters is float64."""
import numpy as np

BINS, DARK, BRIGHT, COUNTERS = 256, 256, 257, 258
OPS = ("film", "reinhard", "aces", "linear")
DEFAULTS = dict(key=0.18, low_fraction=0.05, high_fraction=0.02, ev_bias=0.0, ev_min=-16.0, ev_max=16.0, adapt=1.0, white=4.0)
# log2(1 + (m + 0.5) / 8), m = 0 .. 7: the centres of the eight bins of an octave
CENTRES = np.log2(1.0 + (np.arange(8) + 0.5) / 8.0)


def luminance32(img):
    c = np.asarray(img, dtype=np.float32)
    with np.errstate(all="ignore"):
        return (np.float32(0.3) * c[..., 0] + np.float32(0.6) * c[..., 1]) + np.float32(0.1) * c[..., 2]


def bins_of(lum32):
    """Counter index per value: (bits >> 20) - ((127 - 16) << 3) inside [2^-16, 2^16), DARK for everything that is not >= 2^-16, BRIGHT for
    everything >= 2^16."""
    L = np.asarray(lum32, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        in_lo = L >= np.float32(2.0 ** -16)
        bright = L >= np.float32(2.0 ** 16)
    b = (L.view(np.uint32) >> np.uint32(20)).astype(np.int64) - ((127 - 16) << 3)
    return np.where(~in_lo, DARK, np.where(bright, BRIGHT, b))


def histogram(img):
    idx = bins_of(luminance32(img)).ravel()
    assert idx.min() >= 0 and idx.max() < COUNTERS
    return np.bincount(idx, minlength=COUNTERS).astype(np.uint32)


def auto_ev(hist, have_prev=False, prev_ev=0.0, **params):
    """EV of the 258 counters in float64; the parameters are the float32 fields of spcbpt_display_params."""
    p = dict(DEFAULTS, **params)
    f = {k: np.float64(np.float32(v)) for k, v in p.items()}
    clamp = lambda v: min(max(v, f["ev_min"]), f["ev_max"])
    h = np.asarray(hist[:BINS], dtype=np.uint64)
    N = int(h.sum())
    if N == 0:
        return float(prev_ev) if have_prev else float(clamp(f["ev_bias"]))
    lo = int(f["low_fraction"] * np.float64(N))
    hi = N - int(f["high_fraction"] * np.float64(N))
    end = np.cumsum(h.astype(np.int64))
    start = end - h.astype(np.int64)
    kept = np.clip(np.minimum(end, hi) - np.maximum(start, lo), 0, None)
    b = np.arange(BINS)
    centre = (b >> 3) - 16 + CENTRES[b & 7]
    mean = float(np.dot(kept.astype(np.float64), centre) / kept.sum())
    target = clamp(np.log2(f["key"]) - mean + f["ev_bias"])
    if not have_prev:
        return float(target)
    return float(np.float64(prev_ev) + f["adapt"] * (target - np.float64(prev_ev)))


def tone_codes(img, ev, op, white=4.0):
    """The operator `op` (a name of OPS or its index) on rgb 2^ev in float64, then clamp and sRGB: (..., 3) unrounded codes x 256."""
    op = OPS[op] if not isinstance(op, str) else op
    with np.errstate(all="ignore"):
        c = np.asarray(img, dtype=np.float64)[..., :3] * 2.0 ** np.float64(ev)
        lum = 0.3 * c[..., 0] + 0.6 * c[..., 1] + 0.1 * c[..., 2]
        if op == "film":
            t = c / (1.0 + lum / 1.5)[..., None]
        elif op == "reinhard":
            w = np.float64(np.float32(white))
            t = c * ((1.0 + lum / (w * w)) / (1.0 + lum))[..., None]
        elif op == "aces":
            t = (c * (2.51 * c + 0.03)) / (c * (2.43 * c + 0.59) + 0.14)
        else:
            assert op == "linear"
            t = c
        t = np.clip(t, 0.0, 1.0)
        srgb = np.where(t < 0.0031308, 12.92 * t, 1.055 * np.power(t, 1 / 2.4) - 0.055)
        return np.clip(srgb, 0.0, 1.0) * 256.0


# ------------------------------------------------------------------------------------------------------------ the byte rule
def finite_pixels(img):
    return np.isfinite(np.asarray(img)[..., :3]).all(axis=-1)


def tie_mask(codes):
    """Where a float64 code lies within 1e-3 of an integer in 1 .. 255: float32 arithmetic may land on either side (the tie rule of
    test_gpu_film_buckets.py)."""
    near = np.round(codes)
    return (np.abs(codes - near) < 1e-3) & (near >= 1) & (near <= 255)


def tie_cap(n_values):
    """The most values of an image that may sit at a tie: 2 % of its channel values; 2 values for the two images where that share is
    no whole count to speak of (7 x 5: 105 values, 1 x 1: 3 values)."""
    return max(2, int(0.02 * n_values))


def check_bytes(rgba8, codes, finite):
    """rgba8 against min(floor(codes), 255) at the finite pixels: equal outside the ties, within 1 at them, at most tie_cap of them; alpha
    255 everywhere.  Returns (ties, values that differ) for the caller to print."""
    rgba8 = np.asarray(rgba8)
    assert rgba8.dtype == np.uint8 and rgba8.shape[:-1] == codes.shape[:-1] and rgba8.shape[-1] == 4
    assert (rgba8[..., 3] == 255).all()
    c = codes[finite]
    assert np.isfinite(c).all()
    want = np.minimum(np.floor(c), 255)
    diff = rgba8[..., :3][finite].astype(np.int64) - want
    tie = tie_mask(c)
    ties, cap = int(tie.sum()), tie_cap(c.size)
    assert ties <= cap, (ties, cap)
    assert (diff[~tie] == 0).all(), (int((diff[~tie] != 0).sum()), float(np.abs(diff).max()))
    assert (np.abs(diff) <= 1).all(), float(np.abs(diff).max())
    return ties, int((diff != 0).sum())


# ------------------------------------------------------------------------------------------------------------ the images
SIZES = ((48, 32), (43, 29), (257, 3), (7, 5), (1, 1))   # (width, height)


def seeded_image(width, height, seed=0):
    """2^U(-10, 6) x U(0.2, 1)^3 per pixel, float32, alpha 1: sixteen octaves of luminance, all inside the histogram's range."""
    rng = np.random.default_rng(1000 * width + height + seed)
    scale = 2.0 ** rng.uniform(-10.0, 6.0, (height, width, 1))
    img = np.ones((height, width, 4), np.float32)
    img[..., :3] = (scale * rng.uniform(0.2, 1.0, (height, width, 3))).astype(np.float32)
    return img


def _blue_with_luminance(target):
    """A pixel (0, 0, x) whose float32 luminance, (0 + 0) + 0.1f x, is exactly `target`."""
    t = np.float32(target)
    x = np.float32(t / np.float32(0.1))
    for _ in range(64):
        got = luminance32(np.array([0.0, 0.0, x], np.float32))
        if got == t:
            return (0.0, 0.0, float(x))
        x = np.nextafter(x, np.float32(np.inf) if got < t else np.float32(-np.inf))
    raise AssertionError(f"no float32 blue value has luminance {target!r}")


# the bin edges the edges image straddles, with the bin the edge itself falls in (its float32 predecessor falls in the bin below)
EDGE_BINS = ((2.0 ** -3, 104), (1.125, 129), (1.5, 132), (2.0 ** 10 * 1.875, 215))


def edges_image():
    """16 x 16, hand-built: zero, two negative pixels, a NaN and a +inf pixel, luminance exactly 2^-16 and its float32 predecessor, exactly
    2^16 and its predecessor, both neighbours of four bin edges; the rest seeded and in range.  Returns (image, specials, expected) with
    `specials` the number of leading hand-built pixels and `expected` their counter indices in order."""
    img = seeded_image(16, 16, seed=7)
    flat = img.reshape(-1, 4)
    pred = lambda v: float(np.nextafter(np.float32(v), np.float32(-np.inf)))
    px = [(0.0, 0.0, 0.0), (-0.37, 0.2, -0.11), (-1e-3, -2e-3, -5e-4), (float("nan"), 1.0, 1.0), (float("inf"), 1.0, 1.0)]
    expected = [DARK, DARK, DARK, DARK, BRIGHT]
    for target, where in ((2.0 ** -16, 0), (pred(2.0 ** -16), DARK), (2.0 ** 16, BRIGHT), (pred(2.0 ** 16), 255)):
        px.append(_blue_with_luminance(target))
        expected.append(where)
    for edge, b in EDGE_BINS:
        px.append(_blue_with_luminance(edge))
        expected.append(b)
        px.append(_blue_with_luminance(pred(edge)))
        expected.append(b - 1)
    for i, c in enumerate(px):
        flat[i, :3] = c
    return img, len(px), expected
