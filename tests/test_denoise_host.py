"""spcbpt_denoise_host -- the per-pixel function the denoiser's kernels run (csrc/denoise_pixel.h), on the host -- against a float64
numpy recomputation of the formula in include/spcbpt.h (tests/denoise_ref.py) on synthetic inputs.  Needs no GPU.

Bar: every channel within 1e-4 of the image's largest channel.  An output is a weighted mean of at most 25 taps per iteration, five
iterations: <= 125 float32 accumulations of ~6e-8 each plus a few ulp of expf per weight is ~1e-5; the bar leaves a factor of ten.
Measured: 6.2e-8 (1 iteration) and 7.7e-8 (5 iterations) of the largest channel."""
import ctypes as C

import numpy as np
import pytest

from tests.denoise_ref import atrous_ref

W_, H_ = 43, 29     # no multiple of 8; the step-16 taps of iteration 5 leave the image on every side
SIGMA = (2.0, 0.5, 0.4)
BAR = 1e-4


def _camera():
    t = np.tan(np.radians(20.0))
    eye = np.array([0.3, -0.2, 5.0], np.float32)
    return eye, np.array([t * W_ / H_, 0, 0], np.float32), np.array([0, t, 0], np.float32), np.array([0, 0, -1], np.float32)


def _guides():
    """Two planes with different normals, a depth ramp on each, a sky strip on top, a checker albedo."""
    y, x = np.mgrid[0:H_, 0:W_]
    nd = np.zeros((H_, W_, 4), np.float32)
    left = x < 20
    n1, n2 = np.array([0.6, 0.0, 0.8]), np.array([-0.48, 0.6, 0.64])
    nd[..., :3] = np.where(left[..., None], n1, n2)
    nd[..., 3] = np.where(left, 3.0 + 0.05 * x + 0.02 * y, 4.5 - 0.03 * x + 0.04 * y)
    alb = np.ones((H_, W_, 4), np.float32)
    check = ((x // 4 + y // 4) % 2 == 0)
    alb[..., :3] = np.where(check[..., None], (0.8, 0.6, 0.4), (0.2, 0.3, 0.5))
    sky = y >= H_ - 5
    nd[sky] = 0.0
    alb[sky] = (1.0, 1.0, 1.0, 0.0)
    return alb, nd


@pytest.fixture(scope="module")
def noisy():
    alb, nd = _guides()
    rng = np.random.default_rng(7)
    y, x = np.mgrid[0:H_, 0:W_]
    irradiance = 0.6 + 0.4 * np.sin(x / 9.0) * np.cos(y / 7.0)
    noise = rng.gamma(4.0, 0.25, size=(H_, W_, 3))
    acc = np.ones((H_, W_, 4), np.float32)
    acc[..., :3] = alb[..., :3] * irradiance[..., None] * noise
    return acc, alb, nd


@pytest.mark.parametrize("iterations", [1, 5])
def test_host_filter_matches_float64_formula(pkg, hip_lib, noisy, iterations):
    acc, alb, nd = noisy
    eye, U, V, W = _camera()
    keep = [a.copy() for a in (acc, alb, nd)]
    out = pkg.api.denoise_host(acc, alb, nd, eye, U, V, W, iterations, *SIGMA)
    ref = atrous_ref(acc, alb, nd, U, V, W, iterations, *SIGMA)
    dev = np.abs(out[..., :3] - ref).max() / ref.max()
    print(f"iterations {iterations}: largest deviation {dev:.3e} of the largest channel")
    assert dev <= BAR
    assert np.all(out[..., 3] == 1.0)
    for a, k in zip((acc, alb, nd), keep):   # the inputs are not written
        assert np.array_equal(a, k)
    # the filter did something: it is not the identity on a noisy image
    assert np.abs(out[..., :3] - acc[..., :3]).max() > 0.05


def test_constant_image_comes_back_constant(pkg, hip_lib):
    """Partition of unity: the weights of a pixel sum to one whatever the guides say."""
    alb, nd = _guides()
    alb[..., :3] = 1.0
    acc = np.full((H_, W_, 4), 0.37, np.float32)
    out = pkg.api.denoise_host(acc, alb, nd, *_camera(), 5, *SIGMA)
    assert np.abs(out[..., :3] / 0.37 - 1.0).max() <= 1e-6


def test_demodulation_keeps_the_texture(pkg, hip_lib):
    """radiance = albedo x constant: the filter sees a constant image and hands the checker back unchanged."""
    alb, nd = _guides()
    acc = np.ones((H_, W_, 4), np.float32)
    acc[..., :3] = alb[..., :3] * np.float32(0.7)
    out = pkg.api.denoise_host(acc, alb, nd, *_camera(), 5, *SIGMA)
    assert np.abs(out[..., :3] / acc[..., :3] - 1.0).max() <= 1e-5


def test_defaults_are_taken_for_non_positive_sigmas(pkg, hip_lib, noisy):
    acc, alb, nd = noisy
    a = pkg.api.denoise_host(acc, alb, nd, *_camera(), 3)
    b = pkg.api.denoise_host(acc, alb, nd, *_camera(), 3, -1.0, 0.0, -2.0)
    assert np.array_equal(a, b) and np.isfinite(a).all()


def test_bad_arguments_are_refused(pkg, hip_lib, noisy):
    acc, alb, nd = noisy
    eye, U, V, W = _camera()
    for it in (0, 9):
        with pytest.raises(pkg.SpcbptError, match=r"\(-1\)"):
            pkg.api.denoise_host(acc, alb, nd, eye, U, V, W, it, *SIGMA)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    out = np.zeros_like(acc)
    p = pkg.api.DenoiseParams(2, *SIGMA)
    args = [fp(acc), fp(alb), fp(nd), fp(eye), fp(U), fp(V), fp(W), W_, H_, C.byref(p), fp(out)]
    assert hip_lib.spcbpt_denoise_host(*args) == 0
    for k in (0, 1, 2, 3, 4, 5, 6, 9, 10):
        bad = list(args)
        bad[k] = None
        assert hip_lib.spcbpt_denoise_host(*bad) == -1, k
    assert hip_lib.spcbpt_denoise_params_struct_size() == C.sizeof(pkg.api.DenoiseParams) == 16
