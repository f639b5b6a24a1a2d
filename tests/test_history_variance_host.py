"""spcbpt_history_reproject_var_host / spcbpt_history_resolve_var_host / spcbpt_history_denoise_host -- the per-pixel functions the
variance-carrying kernels of the history reprojection run (csrc/reproject_pixel.h, csrc/denoise_pixel.h), on the host -- against the
float64 restatement of the formulas in include/spcbpt.h (tests/history_var_ref.py) on the analytic two-camera, three-surface scene
of tests/test_reproject_host.py.  Needs no GPU.

Inputs: the history variance HV is a gamma-distributed plane; the moments plane has n = 0, 1, 2 and 7 in its four quadrants (both
branches of the film variance, and the two sides of n = 2), with a sprinkle of M2 a few ulp below zero; the albedo is a checker with
black texels (the floor).

Bar: 1e-4 of the compared plane's largest value, tests/test_reproject_host.py's.  A variance weighted by the prior is compared as
m^2 PV, the quantity the resolve consumes (a ratio of vanishing weights is not comparable across precisions: _weighted there).  PV is
a four-tap weighted mean like the prior's rgb and RV three products and a division on top, so they deviate like the prior (a few
1e-6); the filter is tests/test_film_moments_host.py's with another start value.  The float64 formulas evaluated on these inputs are
printed next to every figure."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import history_var_ref as hv
from tests import reproject_ref as rr
from tests.test_reproject_host import BAR, MAX_HISTORY, SIGMA_N, SIGMA_X, SIZES, _weighted, cameras, image_at, ray_cast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DN_SIGMA = (4.0, 0.5, 40.0)      # sigma_v, sigma_n, sigma_x (scene units: the scene is 556 wide)


def planes(w, h, seed=11):
    """The synthetic planes of one size: features of both views, H, HV, accum, m2n, albedo."""
    rng = np.random.default_rng(seed)
    cur, hist = cameras(w, h)
    nd, sid = ray_cast(cur, w, h)
    G, sid_h = ray_cast(hist, w, h)
    H = np.zeros((h, w, 4), np.float32)
    H[..., :3] = image_at(rr.positions(hist, G)) * (sid_h > 0)[..., None]
    H[..., 3] = (8.0 + 56.0 * np.arange(w) / w)[None, :]                       # below and above max_history
    HV = np.zeros((h, w, 4), np.float32)
    HV[..., :3] = rng.gamma(2.0, 0.01, size=(h, w, 3))
    acc = rng.gamma(2.0, 0.4, size=(h, w, 4)).astype(np.float32)
    acc[..., 3] = 1.0
    m2n = np.zeros((h, w, 4), np.float32)
    y, x = np.mgrid[0:h, 0:w]
    n = np.select([(y < h // 2) & (x < w // 2), (y < h // 2), (x < w // 2)], [0.0, 1.0, 2.0], 7.0)
    m2n[..., 3] = n
    m2n[..., :3] = rng.gamma(2.0, 0.05, size=(h, w, 3)) * np.maximum(n, 1.0)[..., None]
    m2n[::5, ::7, :3] = -1e-7                                                  # max(M2, 0)
    alb = np.zeros((h, w, 4), np.float32)
    alb[..., :3] = np.where(((x // 5 + y // 4) % 2 == 0)[..., None], (0.8, 0.7, 0.6), (0.25, 0.3, 0.5))
    alb[::6, ::5, :3] = 0.0                                                    # a black texel: the floor
    alb[..., 3] = sid > 0
    return dict(w=w, h=h, cur=cur, hist=hist, nd=nd, sid=sid, G=G, sid_h=sid_h, H=H, HV=HV, acc=acc, m2n=m2n, alb=alb)


@pytest.fixture(scope="module", params=SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def case(request, pkg, hip_lib):
    d = planes(*request.param)
    args = (d["cur"], d["nd"], d["hist"], d["G"], d["H"])
    keep = {k: d[k].copy() for k in ("nd", "G", "H", "HV", "acc", "m2n", "alb")}
    d["prior"], d["pv"] = pkg.api.history_reproject_var_host(*args, d["HV"], SIGMA_N, SIGMA_X, MAX_HISTORY)
    d["plain"] = pkg.api.history_reproject_host(*args, SIGMA_N, SIGMA_X, MAX_HISTORY)
    d["ref_prior"], d["ref_pv"] = hv.prior_variance_ref(*args, d["HV"], SIGMA_N, SIGMA_X, MAX_HISTORY)
    d["res"], d["rv"] = pkg.api.history_resolve_var_host(d["prior"], d["pv"], d["acc"], d["m2n"], 3)
    for k, v in keep.items():   # the inputs are not written
        assert np.array_equal(d[k], v), k
    return d


def test_prior_variance_matches_float64_formula(case):
    d = case
    m, m_ref = d["prior"][..., 3:4].astype(np.float64), d["ref_prior"][..., 3:4]
    got, ref = m * m * d["pv"][..., :3], m_ref * m_ref * d["ref_pv"]
    dev = np.abs(got - ref).max() / ref.max()
    print(f"{d['w']}x{d['h']}: m^2 PV, host - float64 {dev:.3g} (of the largest value {ref.max():.3g})")
    assert np.isfinite(d["pv"]).all() and (d["pv"] >= 0).all() and (d["pv"][..., 3] == 0).all()
    assert dev <= BAR
    # the prior beside it is spcbpt_history_reproject_host's, bit for bit
    assert d["prior"].tobytes() == d["plain"].tobytes()
    # PV = 0 wherever R = 0, and the case has both kinds of pixel
    dead = (d["prior"] == 0).all(-1)
    assert (d["pv"][dead] == 0).all() and dead.sum() >= 8 and (~dead).mean() > 0.4
    assert (d["pv"][~dead][..., :3].max(-1) > 0).all()


def test_identity_cameras_hand_the_history_variance_back(case, pkg):
    d = case
    cur, nd, sid = d["cur"], d["nd"], d["sid"]
    H = d["H"].copy()
    H[..., :3] = image_at(rr.positions(cur, nd)) * (sid > 0)[..., None]
    R, PV = pkg.api.history_reproject_var_host(cur, nd, cur, nd, H, d["HV"], SIGMA_N, SIGMA_X, MAX_HISTORY)
    cov = sid > 0
    dev = np.abs(PV[..., :3].astype(np.float64) - d["HV"][..., :3])[cov].max() / d["HV"][..., :3].max()
    print(f"{d['w']}x{d['h']}: identity, largest |PV - HV| on covered pixels {dev:.3g} of the largest HV")
    assert cov.sum() > cov.size // 2
    assert dev <= BAR
    assert (PV[~cov] == 0).all() and (R[~cov] == 0).all()


@pytest.mark.parametrize("frames", [1, 3, 64])
def test_resolved_variance_matches_float64_formula(case, pkg, frames):
    d = case
    res, rv = pkg.api.history_resolve_var_host(d["prior"], d["pv"], d["acc"], d["m2n"], frames)
    ref = hv.resolve_variance_ref(d["prior"], d["pv"], d["acc"], d["m2n"], frames)
    dev = np.abs(rv[..., :3] - ref).max() / ref.max()
    va = hv.film_variance_ref(d["acc"], d["m2n"])
    print(f"{d['w']}x{d['h']}: RV({frames}), host - float64 {dev:.3g} (of the largest value {ref.max():.3g}; largest VA {va.max():.3g})")
    assert np.isfinite(rv).all() and (rv[..., 3] == 0).all()
    assert dev <= BAR
    assert res.tobytes() == pkg.api.history_resolve_host(d["prior"], d["acc"], frames).tobytes()
    live = d["prior"][..., 3] > 3
    assert live.mean() > 0.3 and np.abs(rv[..., :3] - va)[live].max() > 1e-3 * va.max()     # the prior counts


def test_without_a_prior_the_variance_is_the_films(case, pkg):
    d = case
    n = d["m2n"][..., 3]
    assert all((n == k).sum() > 50 for k in (0, 1, 2, 7))
    for frames in (1, 5):
        res, rv = pkg.api.history_resolve_var_host(None, None, d["acc"], d["m2n"], frames)
        # VA in float32, operation for operation: the two lines of the definition
        nn = n * (n - np.float32(1))
        with np.errstate(all="ignore"):
            known = np.maximum(d["m2n"][..., :3], np.float32(0)) / nn[..., None]
        va32 = np.where((n >= 2)[..., None], known, d["acc"][..., :3] * d["acc"][..., :3]).astype(np.float32)
        assert rv[..., :3].tobytes() == va32.tobytes() and (rv[..., 3] == 0).all()
        assert res.tobytes() == pkg.api.history_resolve_host(None, d["acc"], frames).tobytes()
        ref = hv.film_variance_ref(d["acc"], d["m2n"])
        assert np.abs(rv[..., :3] - ref).max() <= BAR * ref.max()
    # sqrtf(VA_k) is the film's standard error of the mean, bit for bit (spcbpt_film_error's sd_k)
    ok = n >= 2
    sd = np.sqrt(np.maximum(d["m2n"][..., :3], np.float32(0))[ok] / (n * (n - np.float32(1)))[ok][:, None])
    assert np.sqrt(rv[..., :3][ok]).tobytes() == sd.astype(np.float32).tobytes()
    assert (rv[::5, ::7][ok[::5, ::7]] == 0).all()                             # M2 below zero: no variance, not a negative one


@pytest.mark.parametrize("iterations", [1, 5])
def test_history_denoise_matches_float64_formula(case, pkg, iterations):
    d = case
    eye, U, V, W = d["cur"]
    keep = [d[k].copy() for k in ("res", "rv", "alb", "nd")]
    out = pkg.api.history_denoise_host(d["res"], d["rv"], d["alb"], d["nd"], eye, U, V, W, iterations, *DN_SIGMA)
    ref = hv.history_denoise_ref(d["res"], d["rv"], d["alb"], d["nd"], U, V, W, iterations, *DN_SIGMA)
    dev = np.abs(out[..., :3] - ref).max() / ref.max()
    print(f"{d['w']}x{d['h']}: history denoise, {iterations} iterations: host - float64 {dev:.3g} of the largest channel {ref.max():.3g}")
    assert np.isfinite(out).all() and (out[..., 3] == 1).all()
    assert dev <= BAR
    for k, v in zip(("res", "rv", "alb", "nd"), keep):
        assert np.array_equal(d[k], v), k
    assert np.abs(out[..., :3] - d["res"][..., :3]).max() > 0.05              # it filtered


@pytest.mark.parametrize("iterations", [1, 5])
def test_known_variance_and_no_prior_is_denoise_variance_bit_for_bit(case, pkg, iterations):
    """The required property: every pixel with n >= 2, no prior live -- the history denoiser is spcbpt_denoise_variance_host."""
    d = case
    eye, U, V, W = d["cur"]
    m2n = d["m2n"].copy()
    m2n[..., 3] = np.where(m2n[..., 3] < 2, 5.0, m2n[..., 3])
    res, rv = pkg.api.history_resolve_var_host(None, None, d["acc"], m2n, 4)
    a = pkg.api.history_denoise_host(res, rv, d["alb"], d["nd"], eye, U, V, W, iterations, *DN_SIGMA)
    b = pkg.api.denoise_variance_host(d["acc"], m2n, d["alb"], d["nd"], eye, U, V, W, iterations, *DN_SIGMA)
    assert a.tobytes() == b.tobytes()
    assert np.abs(a[..., :3] - d["acc"][..., :3]).max() > 0.05
    # defaults: a sigma <= 0 takes denoise_variance's
    a = pkg.api.history_denoise_host(res, rv, d["alb"], d["nd"], eye, U, V, W, 3)
    b = pkg.api.history_denoise_host(res, rv, d["alb"], d["nd"], eye, U, V, W, 3, -1.0, 0.0, -2.0)
    c = pkg.api.denoise_variance_host(d["acc"], m2n, d["alb"], d["nd"], eye, U, V, W, 3)
    assert a.tobytes() == b.tobytes() == c.tobytes()


def test_argument_errors(case, pkg, hip_lib):
    d = case
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    w, h, n = d["w"], d["h"], d["w"] * d["h"]
    out, out_var = np.zeros_like(d["nd"]), np.zeros_like(d["nd"])
    p = pkg.api.ReprojectParams(SIGMA_N, SIGMA_X, MAX_HISTORY)
    args = [fp(v) for v in d["cur"]] + [fp(d["nd"])] + [fp(v) for v in d["hist"]] + [fp(d["G"]), fp(d["H"]), fp(d["HV"]), w, h, C.byref(p), C.c_float(0.0), fp(out), fp(out_var)]
    assert hip_lib.spcbpt_history_reproject_var_host(*args) == 0
    assert out.tobytes() == d["prior"].tobytes() and out_var.tobytes() == d["pv"].tobytes()
    for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 14, 16, 17):
        bad = list(args)
        bad[k] = None
        assert hip_lib.spcbpt_history_reproject_var_host(*bad) == -1, k
    for k, v in ((12, 0), (13, 0)):                                            # an empty image
        bad = list(args)
        bad[k] = v
        assert hip_lib.spcbpt_history_reproject_var_host(*bad) == -1, k
    for nan in ((np.nan, 1.0, 1.0), (1.0, np.nan, 1.0), (1.0, 1.0, np.nan)):
        with pytest.raises(pkg.SpcbptError, match=r"\(-1\)"):
            pkg.api.history_reproject_var_host(d["cur"], d["nd"], d["hist"], d["G"], d["H"], d["HV"], *nan)
    rargs = [fp(d["prior"]), fp(d["pv"]), fp(d["acc"]), fp(d["m2n"]), 3, n, fp(out), fp(out_var)]
    assert hip_lib.spcbpt_history_resolve_var_host(*rargs) == 0
    assert out.tobytes() == d["res"].tobytes() and out_var.tobytes() == d["rv"].tobytes()
    for k, v in ((0, None), (1, None), (2, None), (3, None), (6, None), (7, None), (4, 0), (5, 0)):   # one of prior / prior_var only, NULL, frames == 0, empty
        bad = list(rargs)
        bad[k] = v
        assert hip_lib.spcbpt_history_resolve_var_host(*bad) == -1, k
    with pytest.raises(pkg.SpcbptError, match=r"\(-1\)"):
        pkg.api.history_resolve_var_host(d["prior"], d["pv"], d["acc"], d["m2n"], 0)
    dp = pkg.api.DenoiseParams(2, *DN_SIGMA)
    dargs = [fp(d["res"]), fp(d["rv"]), fp(d["alb"]), fp(d["nd"])] + [fp(v) for v in d["cur"]] + [w, h, C.byref(dp), fp(out)]
    assert hip_lib.spcbpt_history_denoise_host(*dargs) == 0
    for k in (0, 1, 2, 3, 4, 5, 6, 7, 10, 11):
        bad = list(dargs)
        bad[k] = None
        assert hip_lib.spcbpt_history_denoise_host(*bad) == -1, k
    for k in (8, 9):
        bad = list(dargs)
        bad[k] = 0
        assert hip_lib.spcbpt_history_denoise_host(*bad) == -1, k
    for it in (0, 9):
        with pytest.raises(pkg.SpcbptError, match=r"\(-1\)"):
            pkg.api.history_denoise_host(d["res"], d["rv"], d["alb"], d["nd"], *d["cur"], it, *DN_SIGMA)
    sizes = (C.c_int32 * 32)()
    assert hip_lib.spcbpt_abi_struct_sizes(sizes, 32) == 13                    # no new struct


def test_native_program_under_sanitizers(pkg, hip_lib, tmp_path):
    """tests/native/history_var_check.cpp -- the three host forms in a program of its own, every plane in a heap block of its exact
    size -- built with AddressSanitizer and UndefinedBehaviorSanitizer and run on the CPU at 43 x 29: no report, and the bits of the
    library's own host forms."""
    w, h = 43, 29
    exe, fin, fout = (str(tmp_path / n) for n in ("history_var_check", "in.bin", "out.bin"))
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "native", "history_var_check.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    d = planes(w, h, seed=5)
    with open(fin, "wb") as f:
        for a in tuple(d["cur"]) + tuple(d["hist"]) + (np.array([SIGMA_N, SIGMA_X, MAX_HISTORY], np.float32), np.array(DN_SIGMA, np.float32)) + \
                tuple(d[k] for k in ("nd", "G", "H", "HV", "acc", "m2n", "alb")):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    r = subprocess.run([exe, fin, fout, str(w), str(h)], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    prior, pv, res, rv, film, va, den = np.fromfile(fout, np.float32).reshape(7, h, w, 4)
    args = (d["cur"], d["nd"], d["hist"], d["G"], d["H"])
    want_prior, want_pv = pkg.api.history_reproject_var_host(*args, d["HV"], SIGMA_N, SIGMA_X, MAX_HISTORY)
    ref = _weighted(rr.reproject_ref(*args, SIGMA_N, SIGMA_X, MAX_HISTORY))
    assert np.abs(_weighted(prior) - ref).max() <= BAR * ref.max()
    assert np.array_equal(prior, want_prior) and np.array_equal(pv, want_pv)
    want_res, want_rv = pkg.api.history_resolve_var_host(want_prior, want_pv, d["acc"], d["m2n"], 3)
    assert np.array_equal(res, want_res) and np.array_equal(rv, want_rv)
    want_film, want_va = pkg.api.history_resolve_var_host(None, None, d["acc"], d["m2n"], 1)
    assert np.array_equal(film, want_film) and np.array_equal(va, want_va)
    assert film[..., :3].tobytes() == d["acc"][..., :3].tobytes()
    assert np.array_equal(den, pkg.api.history_denoise_host(want_res, want_rv, d["alb"], d["nd"], *d["cur"], 3, *DN_SIGMA))
