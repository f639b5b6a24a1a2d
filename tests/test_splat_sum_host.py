"""spcbpt_splat_sum_host -- the ordered per-pixel sum of the "lt" estimator's ordered mode (csrc/splat_pixel.h, the header k_lt_gather
runs), on the host -- against a numpy loop of np.float32 additions, bit for bit.  Needs no GPU.

The definition (include/spcbpt.h): a pixel's radiance is, per channel, +0.0f plus the rgb of its records in ascending record index, one
float32 addition per record.  The records here span 1e-6 .. 1e3 (log-uniform), so that the order of the additions shows in the last
bits; one pixel receives 5 000 of them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 13, 7
HOT = 5 * W + 4          # the pixel that receives 5 000 records
N_HOT, N_REST = 5000, 3000
EMPTY = 2 * W + 9        # a pixel that receives none


def records(seed=11):
    """(rgb (n, 3) float32, pixel (n,) int32): HOT's 5 000 records interleaved with 3 000 on the other pixels (never EMPTY), and
    a share of invalid pixel indices (negative, and >= W * H)."""
    rng = np.random.default_rng(seed)
    n = N_HOT + N_REST
    rgb = (10.0 ** rng.uniform(-6, 3, size=(n, 3))).astype(np.float32)
    pixel = np.empty(n, np.int32)
    slots = rng.permutation(n)
    pixel[slots[:N_HOT]] = HOT
    rest = rng.integers(0, W * H, size=N_REST)
    rest[(rest == HOT) | (rest == EMPTY)] = 0
    pixel[slots[N_HOT:]] = rest
    bad = slots[N_HOT:][:200]
    pixel[bad[:100]] = -1 - rng.integers(0, 1000, size=100)
    pixel[bad[100:]] = W * H + rng.integers(0, 1000, size=100)
    return rgb, pixel


def numpy_sum(rgb, pixel, w, h, order=None):
    """The definition as a loop of np.float32 additions; `order`: the sequence in which the records are taken (default: ascending)."""
    out = np.zeros((w * h, 3), np.float32)
    for i in (range(len(pixel)) if order is None else order):
        p = int(pixel[i])
        if 0 <= p < w * h:
            for k in range(3):
                out[p, k] = np.float32(out[p, k] + rgb[i, k])
    return out.reshape(h, w, 3)


@pytest.fixture(scope="module")
def case():
    rgb, pixel = records()
    return dict(rgb=rgb, pixel=pixel, want=numpy_sum(rgb, pixel, W, H))


def test_the_order_shows_in_the_bits(case):
    """A shuffled order gives other bits at the hot pixel: without this the comparison below could not notice a wrong order."""
    rgb, pixel, want = case["rgb"], case["pixel"], case["want"]
    assert (pixel == HOT).sum() == N_HOT
    assert rgb.min() >= 1e-6 * 0.999 and rgb.max() <= 1e3 * 1.001 and rgb.min() < 1e-5 and rgb.max() > 1e2
    shuffled = numpy_sum(rgb, pixel, W, H, order=np.random.default_rng(5).permutation(len(pixel)))
    y, x = divmod(HOT, W)
    assert shuffled[y, x].tobytes() != want[y, x].tobytes()
    assert np.allclose(shuffled, want, rtol=2 * N_HOT * 2.0 ** -24, atol=0.0)     # ... and only the last bits


def test_host_form_is_the_ordered_sum(case, pkg, hip_lib):
    rgb, pixel, want = case["rgb"], case["pixel"], case["want"]
    keep = (rgb.copy(), pixel.copy())
    got = pkg.api.splat_sum_host(rgb, pixel, W, H)
    assert np.array_equal(rgb, keep[0]) and np.array_equal(pixel, keep[1])        # the inputs are not written
    assert got.shape == (H, W, 3) and got.dtype == np.float32
    assert got.tobytes() == want.tobytes()
    y, x = divmod(EMPTY, W)
    assert got[y, x].tobytes() == np.zeros(3, np.float32).tobytes()               # +0.0, not -0.0
    assert (got.reshape(-1, 3)[np.setdiff1d(np.arange(W * H), pixel)] == 0).all()


def test_nothing_to_add_and_invalid_indices(pkg, hip_lib):
    """n = 0 gives a film of +0.0; records whose pixel is negative or >= width * height are skipped, also when they are all there is."""
    zero = np.zeros((H, W, 3), np.float32).tobytes()
    assert pkg.api.splat_sum_host(np.zeros((0, 3), np.float32), np.zeros(0, np.int32), W, H).tobytes() == zero
    rgb = np.ones((6, 3), np.float32)
    bad = np.array([-1, W * H, W * H + 1, -2 ** 31, 2 ** 31 - 1, -7], np.int32)
    assert pkg.api.splat_sum_host(rgb, bad, W, H).tobytes() == zero
    one = pkg.api.splat_sum_host(rgb, np.array([-1, W * H - 1, 0, W * H, 0, 0], np.int32), W, H).reshape(-1, 3)
    assert (one[0] == 3).all() and (one[-1] == 1).all() and (one[1:-1] == 0).all()
    neg = pkg.api.splat_sum_host(np.array([[-0.0, 0.0, -0.0]], np.float32), np.array([3], np.int32), W, H).reshape(-1, 3)
    assert neg[3].tobytes() == np.zeros(3, np.float32).tobytes()                  # +0 + -0 = +0: the sum starts from +0.0f
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    out = np.zeros((H, W, 3), np.float32)
    assert hip_lib.spcbpt_splat_sum_host(fp(rgb), ip(bad), 6, W, H, fp(out)) == 0
    assert hip_lib.spcbpt_splat_sum_host(None, None, 0, W, H, fp(out)) == 0
    assert hip_lib.spcbpt_splat_sum_host(None, ip(bad), 6, W, H, fp(out)) == -1
    assert hip_lib.spcbpt_splat_sum_host(fp(rgb), None, 6, W, H, fp(out)) == -1
    assert hip_lib.spcbpt_splat_sum_host(fp(rgb), ip(bad), 6, W, H, None) == -1
    assert hip_lib.spcbpt_splat_sum_host(fp(rgb), ip(bad), -1, W, H, fp(out)) == -1
    assert hip_lib.spcbpt_splat_sum_host(fp(rgb), ip(bad), 6, 0, H, fp(out)) == -1
    assert hip_lib.spcbpt_splat_sum_host(fp(rgb), ip(bad), 6, W, 0, fp(out)) == -1
    with pytest.raises(pkg.SpcbptError):
        pkg.api.splat_sum_host(rgb, bad[:5], W, H)


def test_native_program_under_sanitizers(case, pkg, hip_lib, tmp_path):
    """tests/native/splat_sum_check.cpp -- the host form in a program of its own, every array in a heap block of its exact size, plus
    the device's route (pad key, stable sort, one segment sum per pixel) on the host -- built with AddressSanitizer and
    UndefinedBehaviorSanitizer and run on the CPU: no report, the bits of the numpy loop, and the same for n = 0."""
    exe = str(tmp_path / "splat_sum_check")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "native", "splat_sum_check.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    for name, rgb, pixel, want in (("full", case["rgb"], case["pixel"], case["want"]),
                                   ("none", np.zeros((0, 3), np.float32), np.zeros(0, np.int32), np.zeros((H, W, 3), np.float32))):
        fin, fout = str(tmp_path / (name + "_in.bin")), str(tmp_path / (name + "_out.bin"))
        with open(fin, "wb") as f:
            f.write(np.ascontiguousarray(rgb, np.float32).tobytes())
            f.write(np.ascontiguousarray(pixel, np.int32).tobytes())
        r = subprocess.run([exe, fin, fout, str(len(pixel)), str(W), str(H)], capture_output=True, text=True)
        assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
        got = np.fromfile(fout, np.float32).reshape(H, W, 3)
        assert got.tobytes() == want.tobytes(), name
        assert got.tobytes() == pkg.api.splat_sum_host(rgb, pixel, W, H).tobytes(), name
