"""The film's second moment, the film error and the variance-guided a-trous denoiser on the host -- the per-pixel functions the
kernels run (csrc/moments_pixel.h, csrc/denoise_pixel.h) behind spcbpt_film_moments_update_host, spcbpt_film_error_host and
spcbpt_denoise_variance_host -- against float64 numpy recomputations of the formulas in include/spcbpt.h (tests/denoise_var_ref.py)
on synthetic inputs.  Needs no GPU.

Bars.
  update   |M2 - M2_64| <= 1e-4 n max_f x_f^2 per pixel and channel: about n + 1 float32 roundings of 6e-8 (the running mean's) enter a
           product of two differences of size <= max x, i.e. ~1e-5 n max x^2 at n = 32; the bar leaves the usual factor of ten.
           Measured: at most 4.7e-8 of n max x^2 (n = 2 .. 32).
  error    1e-5 relative on mean and max: a float32 square root and two divisions per pixel (~2e-7), summed in double.
           Measured: 1.2e-8 (mean), 4.7e-8 (max).
  filter   every channel within 1e-4 of the image's largest channel, derived as tests/test_denoise_host.py derives its own: an output
           is a weighted mean of at most 25 taps per iteration, five iterations: <= 125 float32 accumulations of ~6e-8 each plus a few
           ulp of expf per weight is ~1e-5.  What is new here is the division of (L(q) - L(p))^2 by the variance: a rounding of
           L(q) - L(p) moves the exponent by 2 dL 6e-8 L / (sigma_v^2 v), which is largest where v is smallest -- and there the
           weight is either ~0 or c(q) - c(p) is itself ~1e-3 L, so the output moves by < 1e-6 L.
           Measured: 1.3e-7 (1 iteration) and 1.4e-7 (5 iterations) of the largest channel -- below 1e-5, so the bar is that file's 1e-4."""
import ctypes as C

import numpy as np
import pytest

from tests.denoise_var_ref import atrous_var_ref, film_error_ref, welford_ref
from tests.test_denoise_host import H_, W_, _camera, _guides

SIGMA = (4.0, 1.0, 0.4)
BAR = 1e-4


def _film(xs):
    """What the film does with the frames xs (frames, ..., 4) float32: the float32 running mean of film_write, and the moment plane of
    spcbpt_film_moments_update_host applied in front of every merge.  Returns (accum, m2n)."""
    import __graft_entry__ as g
    api = g.load_package().api
    acc = np.zeros(xs.shape[1:], np.float32)
    m2n = np.zeros(xs.shape[1:], np.float32)
    for f, x in enumerate(xs):
        api.film_moments_update_host(acc, x, f, m2n)
        if f == 0:
            acc = x.copy()
        else:
            a = np.float32(1.0) / np.float32(f + 1)
            acc = acc + a * (x - acc)           # lerp3, float32 operation for operation
        acc[..., 3] = 1.0
    return acc, m2n


def _frames(n, seed=11, shape=(H_, W_)):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:shape[0], 0:shape[1]]
    base = (0.2 + np.abs(np.sin(x / 5.0) * np.cos(y / 3.0)))[..., None] * np.array([1.0, 0.5, 2.0])
    xs = np.ones((n,) + shape + (4,), np.float32)
    xs[..., :3] = base * rng.gamma(0.7, 1.5, size=(n,) + shape + (3,))
    return xs


# ------------------------------------------------------------------------------------------------------------ the update
@pytest.mark.parametrize("n", [1, 2, 3, 8, 32])
def test_update_matches_welford_in_float64(pkg, hip_lib, n):
    xs = _frames(n)
    acc, m2n = _film(xs)
    mean, m2, count = welford_ref(xs[..., :3])
    assert np.all(m2n[..., 3] == count)                       # n is exact
    bar = 1e-4 * n * (xs[..., :3].astype(np.float64) ** 2).max(axis=0)
    dev = np.abs(m2n[..., :3] - m2)
    print(f"{n} frames: largest |M2 - float64| {dev.max():.3e}, {(dev / (bar / 1e-4)).max():.3e} of n max x^2 (bar 1e-4)")
    assert np.all(dev <= bar)
    if n == 1:
        assert np.all(m2n[..., :3] == 0)
    else:
        assert m2n[..., :3].max() > 0.01                       # it accumulated something


def test_constant_sequence_has_no_variance_and_subframe_zero_restarts(pkg, hip_lib):
    x = _frames(1)[0]
    acc, m2n = _film(np.repeat(x[None], 9, axis=0))
    assert np.all(m2n[..., :3] == 0) and np.all(m2n[..., 3] == 9)
    xs = _frames(5, seed=12)
    acc, m2n = _film(xs)
    assert m2n[..., :3].max() > 0
    keep_acc, keep_x = acc.copy(), xs[2].copy()
    pkg.api.film_moments_update_host(acc, xs[2], 0, m2n)      # subframe 0: the film overwrites, the moments restart
    assert np.all(m2n[..., :3] == 0) and np.all(m2n[..., 3] == 1)
    assert np.array_equal(acc, keep_acc) and np.array_equal(xs[2], keep_x)   # the inputs are not written


def test_update_refuses_bad_arguments(pkg, hip_lib):
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    a = np.zeros((4, 4), np.float32)
    args = [fp(a), fp(a.copy()), 1, 4, fp(a.copy())]
    assert hip_lib.spcbpt_film_moments_update_host(*args) == 0
    for k in (0, 1, 4):
        bad = list(args)
        bad[k] = None
        assert hip_lib.spcbpt_film_moments_update_host(*bad) == -1, k
    for n in (0, -3, (1 << 28) + 1):
        bad = list(args)
        bad[3] = n
        assert hip_lib.spcbpt_film_moments_update_host(*bad) == -1, n
    with pytest.raises(pkg.SpcbptError):
        pkg.api.film_moments_update_host(a, a, 1, np.zeros((4, 4), np.float64))


# ------------------------------------------------------------------------------------------------------------ the error
def test_error_matches_numpy_in_float64(pkg, hip_lib):
    acc, m2n = _film(_frames(8))
    m2n[3:9, 5:17, 3] = 1.0          # pixels the estimate must leave out ...
    m2n[20:, 30:, 3] = 0.0
    m2n[10, 10, 0] = -1e-9           # ... and a sum of products that rounding left below zero
    got = pkg.api.film_error_host(acc, m2n)
    pixels, mean, top = film_error_ref(acc, m2n)
    print(f"film error: mean {got['mean']:.6g} (float64 {mean:.6g}, rel {abs(got['mean'] / mean - 1):.2e}), "
          f"max {got['max']:.6g} (float64 {top:.6g}, rel {abs(got['max'] / top - 1):.2e}) over {pixels} pixels")
    assert got["pixels"] == pixels == W_ * H_ - 6 * 12 - (H_ - 20) * (W_ - 30)
    assert abs(got["mean"] / mean - 1) <= 1e-5 and abs(got["max"] / top - 1) <= 1e-5
    assert 0 < got["mean"] < got["max"]


def test_error_of_a_film_without_two_samples_is_zero(pkg, hip_lib):
    acc, m2n = _film(_frames(1))
    assert pkg.api.film_error_host(acc, m2n) == {"pixels": 0, "mean": 0.0, "max": 0.0}
    assert hip_lib.spcbpt_film_error_struct_size() == C.sizeof(pkg.api.FilmErrorStats) == 24
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    out = pkg.api.FilmErrorStats()
    args = [fp(acc), fp(m2n), W_ * H_, C.byref(out)]
    assert hip_lib.spcbpt_film_error_host(*args) == 0
    for k in (0, 1, 3):
        bad = list(args)
        bad[k] = None
        assert hip_lib.spcbpt_film_error_host(*bad) == -1, k
    bad = list(args)
    bad[2] = 0
    assert hip_lib.spcbpt_film_error_host(*bad) == -1


def test_error_halves_when_the_frames_quadruple(pkg, hip_lib):
    """What the estimate is for: the standard error of a mean falls like 1 / sqrt(n)."""
    xs = _frames(64, seed=5)
    e16 = pkg.api.film_error_host(*_film(xs[:16]))["mean"]
    e64 = pkg.api.film_error_host(*_film(xs))["mean"]
    print(f"mean relative standard error: {e16:.4f} at 16 frames, {e64:.4f} at 64 (ratio {e64 / e16:.3f})")
    assert 0.4 < e64 / e16 < 0.6


# ------------------------------------------------------------------------------------------------------------ the filter
@pytest.fixture(scope="module")
def noisy():
    """8 frames of the synthetic scene of tests/test_denoise_host.py (gamma noise per channel), as the film and its moments hold them;
    a strip of pixels keeps n = 1 (the branch of the start value)."""
    alb, nd = _guides()
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:H_, 0:W_]
    irradiance = 0.6 + 0.4 * np.sin(x / 9.0) * np.cos(y / 7.0)
    xs = np.ones((8, H_, W_, 4), np.float32)
    xs[..., :3] = alb[..., :3] * irradiance[..., None] * rng.gamma(1.0, 1.0, size=(8, H_, W_, 3))
    acc, m2n = _film(xs)
    m2n[:, 36:] = (0.0, 0.0, 0.0, 1.0)
    return acc, m2n, alb, nd


@pytest.mark.parametrize("iterations", [1, 5])
def test_host_filter_matches_float64_formula(pkg, hip_lib, noisy, iterations):
    acc, m2n, alb, nd = noisy
    eye, U, V, W = _camera()
    keep = [a.copy() for a in noisy]
    out = pkg.api.denoise_variance_host(acc, m2n, alb, nd, eye, U, V, W, iterations, *SIGMA)
    ref = atrous_var_ref(acc, m2n, alb, nd, U, V, W, iterations, *SIGMA)
    dev = np.abs(out[..., :3] - ref).max() / ref.max()
    print(f"iterations {iterations}: largest deviation {dev:.3e} of the largest channel")
    assert dev <= BAR
    assert np.all(out[..., 3] == 1.0)
    for a, k in zip(noisy, keep):   # the inputs are not written
        assert np.array_equal(a, k)
    assert np.abs(out[..., :3] - acc[..., :3]).max() > 0.05    # it filtered


def test_constant_image_comes_back_constant(pkg, hip_lib, noisy):
    alb, nd = _guides()
    alb[..., :3] = 1.0
    acc = np.full((H_, W_, 4), 0.37, np.float32)
    out = pkg.api.denoise_variance_host(acc, noisy[1], alb, nd, *_camera(), 5, *SIGMA)
    assert np.abs(out[..., :3] / 0.37 - 1.0).max() <= 1e-6


def test_demodulation_keeps_the_texture(pkg, hip_lib, noisy):
    """radiance = albedo x constant: the filter sees a constant image and hands the checker back unchanged, whatever the variance says."""
    alb, nd = _guides()
    acc = np.ones((H_, W_, 4), np.float32)
    acc[..., :3] = alb[..., :3] * np.float32(0.7)
    out = pkg.api.denoise_variance_host(acc, noisy[1], alb, nd, *_camera(), 5, *SIGMA)
    assert np.abs(out[..., :3] / acc[..., :3] - 1.0).max() <= 1e-5


def test_defaults_and_bad_arguments(pkg, hip_lib, noisy):
    acc, m2n, alb, nd = noisy
    eye, U, V, W = _camera()
    a = pkg.api.denoise_variance_host(acc, m2n, alb, nd, eye, U, V, W, 3)
    b = pkg.api.denoise_variance_host(acc, m2n, alb, nd, eye, U, V, W, 3, -1.0, 0.0, -2.0)
    assert np.array_equal(a, b) and np.isfinite(a).all()
    for it in (0, 9):
        with pytest.raises(pkg.SpcbptError, match=r"\(-1\)"):
            pkg.api.denoise_variance_host(acc, m2n, alb, nd, eye, U, V, W, it, *SIGMA)
    fp = lambda v: v.ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros_like(acc)
    p = pkg.api.DenoiseParams(2, *SIGMA)
    args = [fp(acc), fp(m2n), fp(alb), fp(nd), fp(eye), fp(U), fp(V), fp(W), W_, H_, C.byref(p), fp(out)]
    assert hip_lib.spcbpt_denoise_variance_host(*args) == 0
    for k in (0, 1, 2, 3, 4, 5, 6, 7, 10, 11):
        bad = list(args)
        bad[k] = None
        assert hip_lib.spcbpt_denoise_variance_host(*bad) == -1, k


# ------------------------------------------------------------------------------------------------------------ what it is for
def _consistency_scene(frames):
    """The scene of the float64 prototype behind the feature: the guides of tests/test_denoise_host.py, a shadow edge inside one plane,
    heavy noise common to the channels, a quiet region on the left."""
    alb, nd = _guides()
    rng = np.random.default_rng(3)
    y, x = np.mgrid[0:H_, 0:W_]
    irr = (0.6 + 0.4 * np.sin(x / 9.0) * np.cos(y / 7.0)) * np.where(x > 30, 2.5, 1.0)
    truth = alb[..., :3] * irr[..., None]
    noise = rng.gamma(0.5, 2.0, size=(frames, H_, W_, 1)) * np.ones(3)
    noise = np.where((x < 10)[None, ..., None], 1.0 + 0.02 * (noise - 1.0), noise)
    xs = np.ones((frames, H_, W_, 4), np.float32)
    xs[..., :3] = truth[None] * noise
    return xs, alb, nd, truth


def _rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - b) ** 2)))


def test_guided_filter_is_consistent_where_the_plain_one_is_not(pkg, hip_lib):
    """At 256 frames the variance-guided filter is closer to the noiseless truth than the film it was given, and the plain a-trous
    filter is farther; at 4 frames the guided filter still helps.  (The float64 formulas alone: 0.0264 / 0.0571 / 0.0888 and
    0.136 / 0.420.)"""
    eye, U, V, W = _camera()
    xs, alb, nd, truth = _consistency_scene(256)
    acc, m2n = _film(xs)
    guided = pkg.api.denoise_variance_host(acc, m2n, alb, nd, eye, U, V, W, 5, *SIGMA)
    plain = pkg.api.denoise_host(acc, alb, nd, eye, U, V, W, 5, *SIGMA)
    noisy_e, guided_e, plain_e = _rmse(acc[..., :3], truth), _rmse(guided[..., :3], truth), _rmse(plain[..., :3], truth)
    ref_e = _rmse(atrous_var_ref(acc, m2n, alb, nd, U, V, W, 5, *SIGMA), truth)
    print(f"256 frames: RMSE noisy {noisy_e:.4f}, guided {guided_e:.4f} (float64 formula {ref_e:.4f}), plain {plain_e:.4f}")
    assert guided_e < noisy_e < plain_e
    acc, m2n = _film(xs[:4])
    guided = pkg.api.denoise_variance_host(acc, m2n, alb, nd, eye, U, V, W, 5, *SIGMA)
    noisy_e, guided_e = _rmse(acc[..., :3], truth), _rmse(guided[..., :3], truth)
    print(f"4 frames: RMSE noisy {noisy_e:.4f}, guided {guided_e:.4f}")
    assert guided_e < noisy_e
