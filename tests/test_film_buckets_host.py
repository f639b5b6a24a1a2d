"""The bucket film and its median-of-means resolve on the host -- the per-pixel functions the kernels run (csrc/buckets_pixel.h) behind
spcbpt_film_buckets_update_host and spcbpt_robust_resolve_host -- against float64 numpy restatements of the definitions in
include/spcbpt.h, on synthetic inputs.  Needs no GPU.

Bars.
  update   every bucket mean within 1e-5 of the pixel's largest sample of the float64 arithmetic mean of the samples with
           subframe % K == b; the counts exact.  Derived: a running mean of n <= 12 float32 steps (48 subframes, K >= 4) accumulates
           at most about 2 n 2^-24 = 1.4e-6 of the largest sample.
  resolve  w equal at every pixel, rgb within 1e-5 of the resolved pixel's largest channel: a sum of at most 32 non-negative float32
           products and one division, ~33 roundings of 6e-8 = 2e-6.  w is an integer decision; the test therefore asserts, on the
           float64 side and at EVERY pixel, that the decision is not a matter of rounding: any two luminance keys of a pixel are
           exactly equal or at least 1e-4 relative apart (float32 keys carry ~2e-7), and t is at least 1e-3 from every integer
           that floorf(t) can cross, 1, 2, ... (t <= 128 carries ~1e-4 at most).  The integer 0 cannot be crossed: G is clamped to
           [0, 1], so t >= 0 in both precisions -- strength 0, k < 3, T == 0 and equal keys (where N is rounding noise around 0)
           all give floorf(t) = 0 on both sides.
  purpose  a constant 0.5 image with single samples of 1000: robust = 0.5 within 1e-6 (the kept buckets hold 0.5 exactly; one division);
           uniform [0.4, 0.6] samples: nothing is trimmed and |robust - float64 mean| <= 1e-6 (64 float32 steps of 6e-8 on 0.5 are
           ~2e-6 worst case, ~2e-7 typical: measured 1.1e-7 on 2 000 pixels)."""
import ctypes as C

import numpy as np
import pytest

INVALID = -1
LUM = np.array([np.float32(0.3), np.float32(0.6), np.float32(0.1)], np.float64)   # the definition's float constants, widened


def _run(api, xs, K, first=0):
    """The planes after the frames xs (frames, ..., 4) merged as subframes first, first + 1, ...: (K, ..., 4) float32."""
    planes = np.zeros((K,) + xs.shape[1:], np.float32)
    for f, x in enumerate(xs):
        api.film_buckets_update_host(x, first + f, planes)
    return planes


def resolve_ref(planes, strength):
    """The definition of include/spcbpt.h in float64 over planes (K, P, 4).  Returns (out (P, 4), t (P,), y (K, P), live (K, P))."""
    p = np.asarray(planes, np.float64)
    K, P = p.shape[:2]
    live = p[..., 3] > 0
    k = live.sum(axis=0)
    y = np.where(live, p[..., :3] @ LUM, 0.0)
    idx = np.arange(K)
    before = (y[None, :, :] < y[:, None, :]) | ((y[None, :, :] == y[:, None, :]) & (idx[None, :, None] < idx[:, None, None]))   # [i, j, p]: j ranks before i
    rank = (before & live[None, :, :]).sum(axis=1)
    T = y.sum(axis=0)
    N = np.where(live, (2 * rank - k + 1) * y, 0.0).sum(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        G = np.where((k >= 3) & (T > 0), np.clip(N / (k * np.where(T > 0, T, 1.0)), 0.0, 1.0), 0.0)
    t = strength * G * k * 0.5
    d = np.minimum((k - 1) // 2, np.floor(t).astype(np.int64))
    d = np.where(k > 0, d, 0)
    kept = live & (rank >= d) & (rank < k - d)
    W = np.where(kept, p[..., 3], 0.0).sum(axis=0)
    S = np.where(kept[..., None], p[..., 3:4] * p[..., :3], 0.0).sum(axis=0)
    out = np.zeros((P, 4))
    some = k > 0
    out[some, :3] = S[some] / W[some, None]
    out[some, 3] = (k - 2 * d)[some]
    return out, t, y, live


# ------------------------------------------------------------------------------------------------------------ the update
@pytest.mark.parametrize("K", [4, 16])
def test_update_matches_the_float64_bucket_means(pkg, hip_lib, K):
    rng = np.random.default_rng(5)
    F, shape = 48, (29, 43)
    xs = np.ones((F,) + shape + (4,), np.float32)
    xs[..., :3] = rng.gamma(0.7, 1.5, size=(F,) + shape + (3,))
    planes = _run(pkg.api, xs, K)
    top = xs[..., :3].astype(np.float64).max(axis=(0, 3))
    worst = 0.0
    for b in range(K):
        mine = xs[b::K, ..., :3].astype(np.float64)
        assert np.all(planes[b, ..., 3] == len(mine))                        # the counts are exact
        dev = np.abs(planes[b, ..., :3] - mine.mean(axis=0)).max(axis=-1)
        worst = max(worst, float((dev / top).max()))
        assert np.all(dev <= 1e-5 * top)
    print(f"K = {K}: largest |bucket mean - float64| {worst:.3e} of the pixel's largest sample (bar 1e-5)")
    # subframe 0 in mid-sequence zeroes every bucket, then fills bucket 0
    pkg.api.film_buckets_update_host(xs[7], 0, planes)
    assert not planes[1:].any()
    assert planes[0, ..., :3].tobytes() == xs[7, ..., :3].tobytes() and np.all(planes[0, ..., 3] == 1)
    # starting at subframe 5 (switched on in mid-film) fills bucket 5 % K
    late = _run(pkg.api, xs[:1], K, first=5)
    assert np.all(late[5 % K, ..., 3] == 1) and late[5 % K, ..., :3].tobytes() == xs[0, ..., :3].tobytes()
    assert not np.delete(late, 5 % K, axis=0).any()


# ------------------------------------------------------------------------------------------------------------ the resolve
def _case_planes(K, per_case=24, seed=11):
    """Synthetic planes (K, P, 4): `per_case` pixels of every case below, each with a colour and a scale of its own.  Within a pixel the
    bucket luminances are multiples m_i of one luminance with the m_i either equal or at least 1 % apart.  (The seed is one of those
    at which no pixel's t comes within 1e-3 of an integer at K = 3, 4, 16, 32 and strengths 0, 1, 4: the test asserts it.)"""
    rng = np.random.default_rng(seed)
    cases = []

    def pixels(mult, n, colour=None):
        """mult, n: (K, per_case); mean_i = mult_i * colour"""
        c = rng.uniform(0.05, 2.0, size=(per_case, 3)) if colour is None else colour
        pl = np.zeros((K, per_case, 4))
        pl[..., :3] = mult[..., None] * c[None]
        pl[..., 3] = n
        cases.append(pl)

    def distinct():   # per pixel a permutation of K multipliers 2 % .. apart, around 1
        base = 1.0 + 0.021 * np.arange(K) * rng.uniform(1.0, 6.0, size=(per_case, 1))
        return np.stack([rng.permutation(row) for row in base], axis=1)

    ones = np.ones((K, per_case))
    pixels(distinct(), 0 * ones)                                                                       # no live bucket
    n = np.zeros((K, per_case)); n[rng.integers(0, K, per_case), np.arange(per_case)] = 4
    pixels(distinct(), n)                                                                              # one live bucket
    n = np.zeros((K, per_case)); n[0] = 2; n[K - 1] = 3
    pixels(distinct(), n)                                                                              # two live buckets
    pixels(ones * rng.uniform(0.5, 2.0, size=(1, per_case)), 4 * ones)                                 # all buckets equal
    m = distinct(); m[rng.integers(0, K, per_case), np.arange(per_case)] *= 1e3
    pixels(m, 4 * ones)                                                                                # one bucket 10^3 times the rest
    F = 2 * K + 3
    pixels(distinct(), (F // K + (np.arange(K) < F % K))[:, None] * ones)                              # unequal n (K = 4: 3, 3, 3, 2)
    live = min(5, K - 1)
    pixels(distinct(), (np.arange(K) < live)[:, None] * ones)                                          # partial fill (K = 16: 5 frames)
    pixels(0 * ones, 4 * ones)                                                                         # a black pixel
    m = distinct(); m[:, : per_case // 2] **= 8
    pixels(m, 4 * ones)                                                                                # spread-out buckets
    planes = np.concatenate(cases, axis=1).astype(np.float32)
    # equal luminance with different colours: (s, 0, 0) and (0, s / 2, 0) have the same key bit for bit in float32 and in float64
    # (0.6 = 2 x 0.3 in both formats), so the index breaks the tie; one brighter bucket makes the trim cut through the tie
    tie = np.zeros((K, per_case, 4), np.float32)
    s = rng.uniform(0.25, 4.0, size=per_case).astype(np.float32)
    tie[0::2, :, 0] = s
    tie[1::2, :, 1] = s * np.float32(0.5)
    where = rng.integers(0, K, per_case)
    tie[where, np.arange(per_case), :3] = (s * np.float32(7.0))[:, None]
    tie[..., 3] = 4
    return np.concatenate([planes, tie], axis=1)


@pytest.mark.parametrize("K", [3, 4, 16, 32])
@pytest.mark.parametrize("strength", [0.0, 1.0, 4.0])
def test_resolve_matches_the_float64_restatement(pkg, hip_lib, K, strength):
    planes = _case_planes(K)
    ref, t, y, live = resolve_ref(planes, strength)
    # the decisions are not a matter of rounding, at every pixel: keys equal or 1e-4 apart, t 1e-3 from the integers 1, 2, ...
    ys = np.sort(np.where(live, y, np.inf), axis=0)
    lo, hi = ys[:-1], ys[1:]
    both = np.isfinite(hi)
    gap = np.where(both, hi - np.where(both, lo, 0.0), 0.0)
    assert np.all((gap == 0) | (gap >= 1e-4 * np.where(both, hi, 1.0)))
    assert np.all(t >= 0)
    near = (np.round(t) >= 1) & (np.abs(t - np.round(t)) < 1e-3)
    assert not near.any(), np.nonzero(near)
    out = pkg.api.robust_resolve_host(planes, strength)
    assert np.all(out[:, 3] == ref[:, 3])                                     # w: equal at every pixel
    top = ref[:, :3].max(axis=1)
    dev = np.abs(out[:, :3] - ref[:, :3]).max(axis=1)
    rel = dev[top > 0] / top[top > 0]
    print(f"K = {K}, strength {strength}: w in {sorted(set(int(v) for v in ref[:, 3]))}, largest |rgb - float64| {rel.max():.3e} of the pixel's largest channel (bar 1e-5)")
    assert np.all(dev <= 1e-5 * top)
    assert not out[top == 0, :3].any()
    if strength == 0.0:   # 0 is the film: every live bucket kept
        assert np.all(ref[:, 3] == live.sum(axis=0))
    if strength == 4.0 and K >= 4:   # ... and the dial does trim
        assert np.any(ref[:, 3] < live.sum(axis=0))


def test_resolve_takes_any_pixel_shape(pkg, hip_lib):
    planes = _case_planes(8)[:, :6 * 7].reshape(8, 6, 7, 4)
    out = pkg.api.robust_resolve_host(planes, 1.0)
    assert out.shape == (6, 7, 4)
    assert out.tobytes() == pkg.api.robust_resolve_host(planes.reshape(8, 42, 4), 1.0).tobytes()


# ------------------------------------------------------------------------------------------------------------ what it is for
def test_fireflies_are_trimmed(pkg, hip_lib):
    rng = np.random.default_rng(9)
    F, K, P = 64, 16, 4000
    xs = np.full((F, P, 4), 0.5, np.float32)
    xs[..., 3] = 1
    hot = rng.choice(P, P // 100, replace=False)
    at = rng.integers(0, F, len(hot))
    at[0] = 37
    xs[at, hot, :3] = 1000.0
    planes = _run(pkg.api, xs, K)
    accum = xs[..., :3].astype(np.float64).mean(axis=0)
    assert np.allclose(accum[hot], 16.1, atol=0.02)
    out = pkg.api.robust_resolve_host(planes, 1.0)
    _, t, _, _ = resolve_ref(planes, 1.0)
    print(f"firefly at subframe 37: t = {t[hot[0]]:.3f}; accum {accum[hot[0], 0]:.3f}, robust {out[hot[0], 0]:.7f}")
    assert abs(t[hot[0]] - 7.27) < 0.01
    assert np.all(out[hot, 3] == 2) and np.all(np.abs(out[hot, :3] - 0.5) <= 1e-6)
    cold = np.ones(P, bool)
    cold[hot] = False
    assert np.all(out[cold, 3] == 16) and np.all(out[cold, :3] == 0.5)


def test_no_harm_where_the_buckets_agree(pkg, hip_lib):
    rng = np.random.default_rng(10)
    F, K, P = 64, 16, 2000
    xs = np.ones((F, P, 4), np.float32)
    xs[..., :3] = rng.uniform(0.4, 0.6, size=(F, P, 3))
    planes = _run(pkg.api, xs, K)
    out = pkg.api.robust_resolve_host(planes, 1.0)
    _, t, _, _ = resolve_ref(planes, 1.0)
    dev = np.abs(out[:, :3] - xs[..., :3].astype(np.float64).mean(axis=0)).max()
    print(f"uniform [0.4, 0.6], 64 frames in 16 buckets: largest t {t.max():.3f}, largest |robust - float64 mean| {dev:.3e}")
    assert np.all(out[:, 3] == 16)
    assert dev <= 1e-6


# ------------------------------------------------------------------------------------------------------------ arguments
def test_bad_arguments_are_refused(pkg, hip_lib):
    fp = C.POINTER(C.c_float)
    x = np.ones((6, 4), np.float32)
    planes = np.zeros((4, 6, 4), np.float32)
    out = np.zeros((6, 4), np.float32)
    px, pp, po = (a.ctypes.data_as(fp) for a in (x, planes, out))
    up, rs = hip_lib.spcbpt_film_buckets_update_host, hip_lib.spcbpt_robust_resolve_host
    assert up(px, 0, 4, 6, pp) == 0 and rs(pp, 4, 6, 1.0, po) == 0
    assert up(None, 0, 4, 6, pp) == INVALID and up(px, 0, 4, 6, None) == INVALID
    assert rs(None, 4, 6, 1.0, po) == INVALID and rs(pp, 4, 6, 1.0, None) == INVALID
    for k in (-1, 0, 1, 2, 33):
        assert up(px, 0, k, 6, pp) == INVALID and rs(pp, k, 6, 1.0, po) == INVALID
    for n in (-1, 0, (1 << 28) + 1):
        assert up(px, 0, 4, n, pp) == INVALID and rs(pp, 4, n, 1.0, po) == INVALID
    for s in (float("nan"), -0.5, 8.5, 9.0, float("inf")):
        assert rs(pp, 4, 6, s, po) == INVALID
    assert rs(pp, 4, 6, 0.0, po) == 0 and rs(pp, 4, 6, 8.0, po) == 0
    with pytest.raises(pkg.SpcbptError):
        pkg.api.film_buckets_update_host(x, 0, np.zeros((2, 6, 4), np.float32))
    with pytest.raises(pkg.SpcbptError):
        pkg.api.robust_resolve_host(planes, 9.0)
    sizes = (C.c_int32 * 32)()
    assert hip_lib.spcbpt_abi_struct_sizes(sizes, 32) == 13                   # no new struct
