"""spcbpt_guide_step_host -- csrc/guide_step.h, the per-bounce arithmetic k_guides runs -- against its definition in float64 (no GPU).

Definition, per record (dir d, normal N turned against the ray, material, a test normal n):
    followed    roughness <= roughness_max and metallic >= metallic_min (both false for a NaN)
    R           d - 2 (N.d) N
    tint        Cspec0 + (1 - Cspec0) (1 - |N.d|)^5,  Cspec0 = lerp(0.08 specular lerp(1, C / lum(C), specular_tint), C, metallic),
                lum = 0.3 r + 0.6 g + 0.1 b (C / lum -> 1 for lum <= 0): the specular Fresnel colour of the Disney BSDF at H = N.
                Sheen does not enter it (the sheen lobe is not specular), so a record has no sheen field; specular and both tints do.
    unfolded    n - 2 (n.N) N

Bars: 4 ulp (float32) of the largest intermediate, from the operation count.
  R, unfolded   the dot product is 3 products and 2 sums of values <= 1 (<= 2.5 half-ulp of 1), doubled exactly; one product <= 2 and one
                difference <= 3 follow.  The largest intermediate is |v_k| + 2 |v.N| |N_k| <= 3 for unit vectors: 4 ulp(3) = 2^-20 = 9.5e-7.
  tint          lum (5 operations), its reciprocal, C / lum (<= 10: pure blue), the three lerps (3 operations each) and the fifth power (4):
                about 20 roundings, each at most half an ulp of the value it produces, all but C / lum and the lerp to it scaled by
                0.08 specular <= 0.08 afterwards.  The largest intermediate of a record is max(1, max_k C_k / lum, max_k lerp(1, C_k / lum,
                specular_tint)); the bar is 4 ulp of it (4.8e-7 for a grey, 3.8e-6 for a pure blue).
  |R| = 1       4 ulp(1) = 4.8e-7 for unit d and N (rounded to float32: their own lengths are 1 to 1.2e-7).
  twice         reflecting n about one plane twice returns n to 4 ulp(3) = 9.5e-7 (two reflections, each within its own bar of the exact one,
                whose square is the identity up to 4 (|N|^2 - 1) <= 4.8e-7 of a float32 unit N, and far less on average).
"""
import numpy as np
import pytest

N_REC = 4096
RMAX, MMIN = np.float32(0.1), np.float32(0.9)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _records(seed=20251, n=N_REC):
    rng = np.random.default_rng(seed)
    d, N, tn = _unit(rng, n), _unit(rng, n), _unit(rng, n)
    flip = (d.astype(np.float64) * N).sum(1) > 0
    N[flip] *= -1                                  # turned against the ray
    mat = rng.random((n, 6)).astype(np.float32)    # base r, g, b, metallic, roughness, specular: the unit box
    st = rng.random(n).astype(np.float32)
    k = n // 8                                     # an eighth each: saturated colours, and the corners of the box
    mat[:k, :3] = np.eye(3, dtype=np.float32)[rng.integers(0, 3, k)] * rng.random((k, 1)).astype(np.float32)
    mat[k:2 * k, 3:] = rng.integers(0, 2, (k, 3)).astype(np.float32)
    st[k:2 * k] = rng.integers(0, 2, k).astype(np.float32)
    return d, N, mat, st, tn


def _truth(d, N, mat, st, tn, rmax=RMAX, mmin=MMIN):
    d, N, mat, st, tn = (np.asarray(x, np.float32).astype(np.float64) for x in (d, N, mat, st, tn))
    cos = (N * d).sum(1)
    R = d - 2.0 * cos[:, None] * N
    unf = tn - 2.0 * (tn * N).sum(1, keepdims=True) * N
    C, metallic, rough, spec = mat[:, :3], mat[:, 3], mat[:, 4], mat[:, 5]
    lum = 0.3 * C[:, 0] + 0.6 * C[:, 1] + 0.1 * C[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        ct = np.where(lum[:, None] > 0, C / lum[:, None], 1.0)
    white = 1.0 + st[:, None] * (ct - 1.0)
    c0 = (0.08 * spec)[:, None] * white
    c0 = c0 + metallic[:, None] * (C - c0)
    F = np.clip(1.0 - np.abs(cos), 0.0, 1.0) ** 5
    tint = c0 + F[:, None] * (1.0 - c0)
    with np.errstate(invalid="ignore"):
        followed = (rough <= float(rmax)) & (metallic >= float(mmin))
    big = np.maximum(1.0, np.maximum(np.abs(ct).max(1), np.abs(white).max(1)))
    return followed, R, tint, unf, big


def _ulp(x):
    return np.spacing(np.asarray(x, np.float32)).astype(np.float64)


def test_step_against_float64(hip_lib, pkg):
    d, N, mat, st, tn = _records()
    followed, R, tint, unf = pkg.api.guide_step_host(d, N, mat, st, tn, RMAX, MMIN)
    f_t, R_t, tint_t, unf_t, big = _truth(d, N, mat, st, tn)
    assert np.array_equal(followed, f_t)
    assert 10 < followed.sum() < N_REC - 10           # both sides of the rule are exercised
    bar = 4 * _ulp(3.0)
    dR, du = np.abs(R - R_t).max(), np.abs(unf - unf_t).max()
    dt = (np.abs(tint - tint_t).max(1) / (4 * _ulp(big))).max()
    print(f"R {dR:.3g}, unfolded {du:.3g} (bar {bar:.3g}); tint {dt:.3g} of its bar (largest intermediate up to {big.max():.3g})")
    assert dR <= bar and du <= bar
    assert dt <= 1.0
    dl = np.abs(np.linalg.norm(R.astype(np.float64), axis=1) - 1.0).max()
    print(f"| |R| - 1 | {dl:.3g} (bar {4 * _ulp(1.0):.3g})")
    assert dl <= 4 * _ulp(1.0)
    _, _, _, back = pkg.api.guide_step_host(d, N, mat, st, unf, RMAX, MMIN)      # the unfolded normal reflected again
    d2 = np.abs(back.astype(np.float64) - tn).max()
    print(f"reflected twice {d2:.3g} (bar {bar:.3g})")
    assert d2 <= bar


def test_thresholds_and_nan(hip_lib, pkg):
    up, down = (lambda x: np.nextafter(np.float32(x), np.float32(2))), (lambda x: np.nextafter(np.float32(x), np.float32(-1)))
    cases = [(RMAX, MMIN, True), (up(RMAX), MMIN, False), (RMAX, down(MMIN), False), (down(RMAX), up(MMIN), True), (0.0, 1.0, True),
             (np.nan, 1.0, False), (0.0, np.nan, False), (np.nan, np.nan, False)]
    n = len(cases)
    d = np.tile(np.float32([0, 0, -1]), (n, 1)); N = np.tile(np.float32([0, 0, 1]), (n, 1))
    mat = np.full((n, 6), 0.5, np.float32)
    mat[:, 4] = [c[0] for c in cases]; mat[:, 3] = [c[1] for c in cases]
    followed, R, _, _ = pkg.api.guide_step_host(d, N, mat, np.zeros(n, np.float32), N, RMAX, MMIN)
    assert followed.tolist() == [c[2] for c in cases]
    assert np.array_equal(R, np.tile(np.float32([0, 0, 1]), (n, 1)))            # head-on: straight back, exactly
    # a threshold below every roughness follows nothing; NaN thresholds follow nothing either
    for rm, mm in ((-1.0, 0.0), (np.nan, 0.0), (1.0, np.nan)):
        f, _, _, _ = pkg.api.guide_step_host(d, N, mat, np.zeros(n, np.float32), N, rm, mm)
        assert not f.any()


def test_head_on_grazing_and_black(hip_lib, pkg):
    """|N.d| = 1: F = 0, the tint is Cspec0; |N.d| = 1e-6: F = (1 - 1e-6)^5, the tint is all but white; a black base (lum = 0) takes C / lum = 1."""
    N = np.tile(np.float32([0, 0, 1]), (3, 1))
    g = np.float32(1e-6)
    d = np.float32([[0, 0, -1], [np.sqrt(1 - np.float64(g) ** 2), 0, -g], [0, 0, -1]])
    mat = np.float32([[0.9, 0.8, 0.7, 1.0, 0.02, 0.5], [0.9, 0.8, 0.7, 1.0, 0.02, 0.5], [0, 0, 0, 0.0, 0.5, 1.0]])
    st = np.float32([0.0, 0.0, 1.0])
    _, R, tint, _ = pkg.api.guide_step_host(d, N, mat, st, N)
    _, R_t, tint_t, _, big = _truth(d, N, mat, st, N)
    assert np.array_equal(tint[0], mat[0, :3])                                  # metallic 1, head-on: the base colour, exactly
    assert np.abs(tint - tint_t).max() <= 4 * _ulp(1.0) and (tint[1] > 0.99999).all()
    assert np.array_equal(tint[2], np.float32([0.08, 0.08, 0.08]))              # 0.08 specular (1 + 1 (1 - 1)) at metallic 0
    assert np.abs(R - R_t).max() <= 4 * _ulp(3.0)
    assert np.abs(np.linalg.norm(R.astype(np.float64), axis=1) - 1.0).max() <= 4 * _ulp(1.0)


def test_bad_arguments_and_exports(hip_lib, pkg):
    d = np.zeros((2, 3), np.float32)
    with pytest.raises(pkg.SpcbptError):
        pkg.api.guide_step_host(d, d, np.zeros((2, 5), np.float32), np.zeros(2, np.float32), d)
    assert hip_lib.spcbpt_guide_step_host(0, None, None, None, None, None, None, None, None, None, None) == -1
    assert hip_lib.spcbpt_guide_params_struct_size() == 12
    import ctypes as C
    assert C.sizeof(pkg.api.GuideParams) == 12
    for name in ("spcbpt_launch_guides", "spcbpt_read_guides", "spcbpt_set_denoise_guides", "spcbpt_guide_params_struct_size", "spcbpt_guide_step_host"):
        assert name in pkg.api.EXPORTED_SYMBOLS and hasattr(hip_lib, name)
