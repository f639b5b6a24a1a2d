"""Adaptive sampling's tile selection on the host (spcbpt_adaptive_select_host: csrc/adaptive_pixel.h over plain arrays, the functions
k_tile_error / k_tile_select run) against a numpy float64 restatement of include/spcbpt.h's definition, on synthetic 43x29 planes:
6 x 4 tiles of 8x8 pixels, the last column 3 pixels wide and the last row 5 pixels high.

Bars: tile errors 1e-5 relative (the bar tests/test_gpu_film_moments.py holds the same per-pixel arithmetic to: a float32 square root,
two divisions and a 64-term float32 sum against float64 -- 64 terms of one sign lose at most 64 x 2^-24 = 4e-6 relative, the per-pixel
term a few 2^-24 more); the lists EQUAL, with the target placed in the middle of a gap of at least 1e-3 relative between two
neighbouring tile errors (a hundred times the bar, so no tile may fall on the other side).  Needs no GPU."""
import ctypes as C

import numpy as np
import pytest

W, H = 43, 29
TX, TY = 6, 4
INVALID = -1
UNKNOWN, BLACK, AT_MAX, BELOW_MIN, MIXED, CORNER = 3, 7, 10, 12, 15, 23
MIN_SAMPLES, MAX_SAMPLES = 4, 64


def tile_slices(t):
    x0, y0 = (t % TX) * 8, (t // TX) * 8
    return slice(y0, min(y0 + 8, H)), slice(x0, min(x0 + 8, W))


def tile_errors_ref(accum, m2n):
    """float64: (e_t, known_t) per tile; e(p) of include/spcbpt.h (spcbpt_film_error), the mean over the in-image pixels with n >= 2."""
    a, m = accum.astype(np.float64), m2n.astype(np.float64)
    n = m[..., 3]
    ok = n >= 2
    nn = np.where(ok, n * (n - 1), 1.0)
    sd = np.sqrt(np.maximum(m[..., :3], 0.0) / nn[..., None])
    lum = 0.3 * a[..., 0] + 0.6 * a[..., 1] + 0.1 * a[..., 2]
    e = (0.3 * sd[..., 0] + 0.6 * sd[..., 1] + 0.1 * sd[..., 2]) / (1e-2 + lum)
    err, known = np.zeros(TX * TY), np.zeros(TX * TY, dtype=np.int64)
    for t in range(TX * TY):
        ys, xs = tile_slices(t)
        k = ok[ys, xs]
        known[t] = int(k.sum())
        err[t] = e[ys, xs][k].mean() if known[t] else 0.0
    return err, known


def select_ref(err, known, samples, target, min_samples, max_samples):
    out = []
    for t in range(TX * TY):
        below_cap = max_samples == 0 or samples[t] < max_samples
        if below_cap and (samples[t] < max(min_samples, 2) or known[t] == 0 or err[t] > target):
            out.append(t)
    return np.array(out, dtype=np.uint32)


def gap_target(err, usable):
    """The middle of the gap of at least 1e-3 relative between two neighbouring sorted tile errors that is nearest to the median."""
    e = np.sort(np.asarray(err, np.float64)[usable])
    e = e[e > 0]
    assert e.size >= 4
    gaps = [(abs(i - e.size // 2), i) for i in range(1, e.size) if e[i] - e[i - 1] >= 1e-3 * e[i]]
    assert gaps, "the inputs hold no gap of 1e-3 relative between neighbouring tile errors"
    i = min(gaps)[1]
    return 0.5 * (e[i - 1] + e[i])


@pytest.fixture(scope="module")
def planes():
    rng = np.random.default_rng(20240607)
    accum = np.zeros((H, W, 4), np.float32)
    accum[..., :3] = rng.uniform(0.05, 2.0, (H, W, 3))
    accum[..., 3] = 1.0
    m2n = np.zeros((H, W, 4), np.float32)
    m2n[..., 3] = 8.0
    for t in range(TX * TY):   # a noise level per tile, a factor 1.25 apart in a shuffled order: gaps far above 1e-3
        ys, xs = tile_slices(t)
        level = 1e-3 * 1.25 ** ((t * 7) % (TX * TY))
        shape = accum[ys, xs, :3].shape
        m2n[ys, xs, :3] = (level * rng.uniform(0.8, 1.2, shape) * accum[ys, xs, :3]) ** 2 * 56.0
    samples = np.full(TX * TY, 8, np.uint32)
    ys, xs = tile_slices(UNKNOWN)
    m2n[ys, xs, 3] = 1.0                                  # no pixel with two samples
    ys, xs = tile_slices(BLACK)
    accum[ys, xs, :3] = 0.0
    m2n[ys, xs, :3] = 0.0                                 # all black: e = 0, and known
    ys, xs = tile_slices(AT_MAX)
    m2n[ys, xs, :3] *= 1e4                                # the noisiest tile of all, but at the cap
    samples[AT_MAX] = MAX_SAMPLES
    ys, xs = tile_slices(BELOW_MIN)
    m2n[ys, xs, :3] *= 1e-6                               # converged, but short of the floor
    samples[BELOW_MIN] = MIN_SAMPLES - 1
    ys, xs = tile_slices(MIXED)
    m2n[ys, xs, 3] = np.where(rng.uniform(size=m2n[ys, xs, 3].shape) < 0.4, 1.0, 8.0)   # some pixels without an estimate
    m2n[0, 0, 0] = -1e-9                                  # a sum of products a few ulp below zero (moments_pixel.h: max(., 0))
    ys, xs = tile_slices(CORNER)
    assert accum[ys, xs].shape[:2] == (5, 3)              # the partial corner tile
    m2n[ys.start, xs.start, 3] = 0.0                      # ... one of its 15 pixels never sampled
    return accum, m2n, samples


def test_struct_size(hip_lib, pkg):
    assert hip_lib.spcbpt_adaptive_params_struct_size() == C.sizeof(pkg.api.AdaptiveParams) == 12
    sizes = (C.c_int32 * 32)()
    assert hip_lib.spcbpt_abi_struct_sizes(sizes, 32) == 13   # no new entry


def test_tile_errors_match_float64(pkg, planes):
    accum, m2n, samples = planes
    err, known = tile_errors_ref(accum, m2n)
    got = pkg.api.adaptive_select_host(accum, m2n, samples, 0.0)["error"]
    assert got.shape == (TY, TX) and got.dtype == np.float32
    got = got.reshape(-1).astype(np.float64)
    assert known[UNKNOWN] == 0 and got[UNKNOWN] == 0.0
    assert known[BLACK] == 64 and got[BLACK] == 0.0 and err[BLACK] == 0.0
    assert known[CORNER] == 14 and 0 < known[MIXED] < 64
    pos = err > 0
    rel = np.abs(got[pos] / err[pos] - 1)
    print(f"tile errors {err[pos].min():.3g} .. {err[pos].max():.3g}; host - float64 at most {rel.max():.3g} relative (bar 1e-5)")
    assert pos.sum() == TX * TY - 2 and np.all(got[~pos] == 0)
    assert rel.max() <= 1e-5


@pytest.mark.parametrize("min_samples,max_samples", [(MIN_SAMPLES, MAX_SAMPLES), (0, 0), (0, MAX_SAMPLES), (9, 0)])
def test_selected_list_equals_float64(pkg, planes, min_samples, max_samples):
    accum, m2n, samples = planes
    err, known = tile_errors_ref(accum, m2n)
    usable = np.ones(TX * TY, bool)
    usable[[UNKNOWN, BLACK, AT_MAX, BELOW_MIN]] = False
    target = gap_target(err, usable)
    want = select_ref(err, known, samples, target, min_samples, max_samples)
    got = pkg.api.adaptive_select_host(accum, m2n, samples.reshape(TY, TX), target, min_samples, max_samples)["tiles"]
    print(f"target {target:.4g}, min {min_samples}, max {max_samples}: {got.size} of {TX * TY} tiles selected")
    assert got.dtype == np.uint32 and got.tolist() == want.tolist()
    assert np.all(np.diff(got.astype(np.int64)) > 0)                   # strictly ascending
    assert (AT_MAX in got) == (max_samples == 0)                        # the noisiest tile: only the cap keeps it out
    assert (BELOW_MIN in got) == (samples[BELOW_MIN] < max(min_samples, 2))
    if min_samples == 9:
        assert got.tolist() == list(range(TX * TY))                    # every tile is short of the floor, none at a cap
    else:
        assert 0 < got.size < TX * TY and UNKNOWN in got and BLACK not in got


def test_extremes_and_optional_outputs(hip_lib, pkg, planes):
    accum, m2n, samples = planes
    every = pkg.api.adaptive_select_host(accum, m2n, samples, -1.0)["tiles"]      # every known tile is above a negative target
    assert every.tolist() == list(range(TX * TY))                                 # (no cap: the tile at 64 samples too)
    none = pkg.api.adaptive_select_host(accum, m2n, samples, np.inf)["tiles"]
    assert none.tolist() == [UNKNOWN]                                             # nothing is above +inf; the unknown tile stays
    zero = pkg.api.adaptive_select_host(accum, m2n, np.zeros(TX * TY, np.uint32), np.inf, 0, 1)["tiles"]
    assert zero.size == TX * TY                                                   # no samples yet: every tile, whatever the film says
    # every output pointer is optional
    p = pkg.api.AdaptiveParams(-1.0, 0, 0)
    n = C.c_int(-7)
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert hip_lib.spcbpt_adaptive_select_host(f(accum), f(m2n), W, H, samples.ctypes.data, C.byref(p), None, None, C.byref(n)) == 0
    assert n.value == TX * TY
    assert hip_lib.spcbpt_adaptive_select_host(f(accum), f(m2n), W, H, samples.ctypes.data, C.byref(p), None, None, None) == 0


def test_bad_arguments_are_refused(hip_lib, pkg, planes):
    accum, m2n, samples = planes
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    p = pkg.api.AdaptiveParams(0.1, 0, 0)
    nan = pkg.api.AdaptiveParams(float("nan"), 0, 0)
    call = hip_lib.spcbpt_adaptive_select_host
    assert call(None, f(m2n), W, H, samples.ctypes.data, C.byref(p), None, None, None) == INVALID
    assert call(f(accum), None, W, H, samples.ctypes.data, C.byref(p), None, None, None) == INVALID
    assert call(f(accum), f(m2n), W, H, None, C.byref(p), None, None, None) == INVALID
    assert call(f(accum), f(m2n), W, H, samples.ctypes.data, None, None, None, None) == INVALID
    assert call(f(accum), f(m2n), 0, H, samples.ctypes.data, C.byref(p), None, None, None) == INVALID
    assert call(f(accum), f(m2n), W, -1, samples.ctypes.data, C.byref(p), None, None, None) == INVALID
    assert call(f(accum), f(m2n), 1 << 15, 1 << 15, samples.ctypes.data, C.byref(p), None, None, None) == INVALID
    assert call(f(accum), f(m2n), W, H, samples.ctypes.data, C.byref(nan), None, None, None) == INVALID
    with pytest.raises(pkg.SpcbptError):
        pkg.api.adaptive_select_host(accum, m2n[:-1], samples, 0.1)
    with pytest.raises(pkg.SpcbptError):
        pkg.api.adaptive_select_host(accum, m2n, samples[:-1], 0.1)
    with pytest.raises(pkg.SpcbptError):
        pkg.api.adaptive_select_host(accum.reshape(-1, 4), m2n.reshape(-1, 4), samples, 0.1)
