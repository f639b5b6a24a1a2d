"""The thin-lens camera on the device (spcbpt_set_lens): "SPCBPT_eye" and "pt" generate lens rays, "lt" connects every cache vertex to a
lens point of its own -- two implementations of one camera that share no camera-side code, so they are held against each other, and
each against the float64 definition of tests/lens_ref.py."""
import hashlib
import math
import os
import subprocess

import numpy as np
import pytest

from tests import lens_ref as L
from tests.lens_film import frame as _frame, host_film
from tests.test_gpu_mesh_light import _light_geometry, _lum, _renderer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, INVALID = -5, -1


def _lens_of(pkg, scene, w, h, share=0.03):
    _, _, _, W = _frame(pkg, scene, w, h)
    return float(np.float32(share * np.linalg.norm(W)))


# ------------------------------------------------------------------------------------------------------------ off means off
def test_radius_zero_leaves_every_film_bit_for_bit(gpu, pkg):
    """Cornell box, 48 x 32, two subframes: after set_lens(0, 3) the films of "SPCBPT_eye", "pt" and "lt" (ordered mode) are, bit for
    bit, those of a context that never called it -- the launchers keep the pinhole kernels, and `focus` is ignored."""
    scene = pkg.scenes.cornell_box()
    films = []
    for lens in (False, True):
        r = _renderer(pkg, scene, 48, 32, light=(2000, 16, 1), tuple_="minimal")
        r.set_splat_order(pkg.api.SPLAT_ORDERED)
        if lens:
            r.set_lens(0.0, 3.0)
            assert r.lens() == (0.0, 3.0)
        else:
            assert r.lens() == (0.0, 0.0)
        out = {}
        for alg in ("SPCBPT_eye", "pt", "lt"):
            r.clear_accum()
            for f in range(2):
                r.render_frame(alg, f)
            r.sync()
            out[alg] = r.read_accum().copy()
            assert np.isfinite(out[alg]).all() and out[alg][..., :3].mean() > 0
        films.append(out)
    for alg in films[0]:
        assert films[0][alg].tobytes() == films[1][alg].tobytes(), alg


def test_set_lens_validates_and_survives_camera_and_resize(gpu, pkg):
    scene = pkg.scenes.cornell_box()
    r = _renderer(pkg, scene, 48, 32, light=(2000, 16, 1), tuple_="minimal")
    for radius, focus in ((-0.1, 1.0), (0.1, 0.0), (0.1, -1.0), (float("nan"), 1.0), (0.1, float("nan")), (float("inf"), 1.0), (0.1, float("inf"))):
        with pytest.raises(pkg.SpcbptError) as e:
            r.set_lens(radius, focus)
        assert f"({INVALID})" in str(e.value) and "set_lens" in str(e.value), str(e.value)
        assert r.lens() == (0.0, 0.0)
    r.set_lens(0.25, 0.75)
    cam = scene.camera
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], 1.0)
    r.resize(32, 32)
    assert r.lens() == (0.25, 0.75)
    # ... and the lens axes followed the new frame: the device's rays are the host form's for the NEW camera
    U, V, W = pkg.camera_frame(cam["eye"], cam["lookat"], cam["up"], cam["fov"], 1.0)
    o, d = r.lens_rays(1)
    s = pkg.api.lens_sample_host(np.arange(32 * 32), 1, True)
    y, x = np.divmod(np.arange(32 * 32), 32)
    ho, hd = pkg.api.camera_lens_ray_host(np.array(cam["eye"], np.float32), U, V, W, 32, 32, np.stack([x, y], 1), s[:, 0:2], s[:, 2:4], 0.25, 0.75)
    assert np.abs(o.reshape(-1, 3) - ho).max() < 1e-6 and np.abs(d.reshape(-1, 3) - hd).max() < 1e-6


# ------------------------------------------------------------------------------------------------------------ device rays
def test_device_rays_against_the_definition(gpu, pkg):
    """Renderer.lens_rays() -- the device function k_pt_lens and k_spcbpt_lens call -- at 48 x 32, subframes 0 and 3, against
    spcbpt_camera_lens_ray_host fed by spcbpt_lens_sample_host, and both against tests/lens_ref.py.  The header evaluates the disc map's
    sine and cosine with polynomial kernels of its own, so host and device share EVERY operation as + - x / sqrt: equal bit for bit.
    The assertion against the float64 definition: the device's worst error is at most 4 x the host form's own on the same inputs.
    Measured on the MI355X: device 1.24e-7, host form 1.24e-7, 0 of 18 432 values differ."""
    scene = pkg.scenes.cornell_box()
    w, h = 48, 32
    r = _renderer(pkg, scene, w, h, light=(2000, 16, 1), tuple_="minimal")
    eye, U, V, W = _frame(pkg, scene, w, h)
    R, focus = _lens_of(pkg, scene, w, h), 0.7
    r.set_lens(R, focus)
    y, x = np.divmod(np.arange(w * h), w)
    for sub in (0, 3):
        o, d = r.lens_rays(sub)
        o, d = o.reshape(-1, 3), d.reshape(-1, 3)
        s = pkg.api.lens_sample_host(np.arange(w * h), sub, True)
        if sub == 0:
            assert (s[:, 0:2] == 0.5).all()
        ho, hd = pkg.api.camera_lens_ray_host(eye, U, V, W, w, h, np.stack([x, y], 1), s[:, 0:2], s[:, 2:4], R, focus)
        O64, d64, _, _ = L.lens_ray(eye, U, V, W, w, h, x, y, s[:, 0], s[:, 1], s[:, 2], s[:, 3], R, focus)
        host_err = max(np.abs(ho - O64).max(), np.abs(hd - d64).max())
        dev_err = max(np.abs(o - O64).max(), np.abs(d - d64).max())
        differ = int((o != ho).sum() + (d != hd).sum())
        print(f"subframe {sub}: device rays against float64 {dev_err:.3g}, host form {host_err:.3g}; values that differ between device and host: {differ} of {o.size + d.size}")
        assert np.isfinite(o).all() and np.isfinite(d).all()
        assert dev_err <= 4 * host_err
        assert o.tobytes() == ho.tobytes() and d.tobytes() == hd.tobytes()
        assert np.linalg.norm(o - eye, axis=1).max() <= R + 1e-5       # inside the lens (to the rounding of eye + offset)


# ------------------------------------------------------------------------------------------------------------ lt: the cache's own sum
@pytest.fixture(scope="module")
def box(gpu, pkg, ob):
    """The Cornell box at 48 x 32 through a lens of 3 % of |W| focused at 0.7: one "lt" frame of 2000 light paths, the cache it read
    and its float64 recount."""
    scene = pkg.scenes.cornell_box()
    w, h = 48, 32
    r = _renderer(pkg, scene, w, h, light=(2000, 16, 1), tuple_="minimal")
    R, focus = _lens_of(pkg, scene, w, h), 0.7
    r.set_lens(R, focus)
    r.render_frame("lt", 0)
    r.sync()
    film = r.read_accum().copy()
    v = r.lvc_read()
    _, _, _, vc, pc = r.sampler_read()
    assert vc == len(v) and pc == 2000
    host = host_film(pkg, ob, r, scene, v, pc, w, h, R, focus)
    return dict(scene=scene, r=r, w=w, h=h, film=film, host=host, lens=(R, focus))


def test_the_lens_film_is_the_caches_own_sum(box):
    """test_the_film_is_the_caches_own_sum of tests/test_gpu_splat.py through the lens: every pixel of one "lt" frame against the float64
    sum over the vertices of the cache the launch read, each seen from the lens point of its own slot (tests/lens_film.py: lens_ref
    and spcbpt_lens_sample_host).  That test's bar, rtol 1e-4, and its way of leaving out pixels that hang on a float32 decision (a
    vertex within 1e-4 pixel of a pixel edge, or grazing its lens point below 1e-3), with its cap of 3 % of the lit pixels
    (tests/test_camera_lens_cpu.py checks the cap on the oracle's cache without a GPU).  Unlit pixels are exactly 0.  Measured on the
    MI355X: largest deviation 1.4e-6, 5 of 501 lit pixels (1.0 %) left out."""
    film, (want, excluded, lit, survivors, total) = box["film"], box["host"]
    got = film[..., :3].astype(np.float64)
    assert np.isfinite(film).all()
    share = (excluded & lit).sum() / max(1, lit.sum())
    print(f"cache: {total} vertices, {survivors} splat ({survivors / total:.3f}); lit pixels {int(lit.sum())}, excluded {int((excluded & lit).sum())} ({share:.4f})")
    assert survivors > 500 and lit.sum() > 300
    assert share <= 0.03, share
    check = ~excluded
    assert (got[check & ~lit] == 0).all(), "a pixel no vertex reaches is not exactly 0"
    sel = check & lit
    dev = np.abs(got[sel] - want[sel]) / want[sel].max(-1, keepdims=True)
    print(f"largest deviation from the float64 sum: {dev.max():.3g} (of the pixel's largest channel)")
    assert np.allclose(got[sel], want[sel], rtol=1e-4, atol=0.0), dev.max()


def test_bands_and_order(box, pkg):
    """"lt" through the lens: rows (0, 16) then (16, 32) against a full launch of the same cache to rtol 1e-5 in the atomic mode (the
    order of the float atomics is the only difference), and bit-equal films in the ordered mode -- full against full, and the two
    bands against full: a slot's lens point depends on the slot and the subframe, not on the thread or the band that looks at it."""
    r = box["r"]
    r.clear_accum()
    r.launch("lt", 0)
    r.sync()
    full = r.read_accum().copy()
    assert np.allclose(full[..., :3], box["film"][..., :3], rtol=1e-5, atol=0.0)
    r.clear_accum()
    r.launch("lt", 0, (0, 16, 1))
    r.launch("lt", 0, (16, 32, 1))
    r.sync()
    b = r.read_accum().copy()
    assert np.allclose(b[..., :3], full[..., :3], rtol=1e-5, atol=0.0)
    assert ((b[..., :3] == 0) == (full[..., :3] == 0)).all()
    r.set_splat_order(pkg.api.SPLAT_ORDERED)
    films = []
    for bands in (None, None, ((0, 16, 1), (16, 32, 1))):
        r.clear_accum()
        for rows in (bands or (None,)):
            r.launch("lt", 0, rows)
        r.sync()
        films.append(r.read_accum().copy())
    r.set_splat_order(pkg.api.SPLAT_ATOMIC)
    r.clear_accum()
    assert films[0].tobytes() == films[1].tobytes() == films[2].tobytes()
    assert np.allclose(films[0][..., :3], full[..., :3], rtol=1e-5, atol=0.0)


# ------------------------------------------------------------------------------------------------------------ three estimators
def _hits(P64, O, d, margin=1e-3):
    """Moeller-Trumbore of rays (O, d) (n, 3 each) against triangles P64 (k, 3, 3): (front-face hit inside the margins, any hit at all
    -- margins turned outwards) per ray, as test_a_seen_emitter_shows_its_radiance selects its pixels."""
    front = np.zeros(len(d), bool)
    anyhit = np.zeros(len(d), bool)
    for k in range(len(P64)):
        e1, e2 = P64[k, 1] - P64[k, 0], P64[k, 2] - P64[k, 0]
        n = np.cross(e1, e2)
        pv = np.cross(d, e2)
        det = pv @ e1
        tv = O - P64[k, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            u = (pv * tv).sum(1) / det
            qv = np.cross(tv, e1)
            v = (d * qv).sum(1) / det
            tt = (qv @ e2) / det
        front |= (d @ n < 0) & (u > margin) & (v > margin) & (u + v < 1 - margin) & (tt > 0)
        anyhit |= (u > -margin) & (v > -margin) & (u + v < 1 + margin) & (tt > 0)
    return front, anyhit


def _cones(eye, U, V, Wv, w, h, R, focus, tris, lamp):
    """Per pixel: does its whole cone -- its four corners crossed with 16 points on the lens rim -- lie on the lamp's front faces, and does
    it miss every triangle of the scene?"""
    y, x = np.mgrid[0:h, 0:w]
    whole, empty = np.ones((h, w), bool), np.ones((h, w), bool)
    ang = 2 * np.pi * np.arange(16) / 16
    rim = R * (np.cos(ang)[:, None] * U / np.linalg.norm(U) + np.sin(ang)[:, None] * V / np.linalg.norm(V))
    for ox, oy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        F = eye + focus * ((2 * (x + ox) / w - 1)[..., None] * U + (2 * (y + oy) / h - 1)[..., None] * V + Wv)
        for k in range(16):
            O = eye + rim[k]
            d = (F - O).reshape(-1, 3)
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            Ob = np.broadcast_to(O, d.shape)
            front, _ = _hits(lamp, Ob, d)
            _, anyhit = _hits(tris, Ob, d)
            whole &= front.reshape(h, w)
            empty &= ~anyhit.reshape(h, w)
    return whole, empty


def _point_triangle_distance(p, tri):
    a, b, c = tri
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n)
    q = p - (p - a) @ n * n
    inside = all(np.cross(v1 - v0, q - v0) @ n >= 0 for v0, v1 in ((a, b), (b, c), (c, a)))
    if inside:
        return abs((p - a) @ n)
    best = np.inf
    for v0, v1 in ((a, b), (b, c), (c, a)):
        t = np.clip((p - v0) @ (v1 - v0) / ((v1 - v0) @ (v1 - v0)), 0, 1)
        best = min(best, np.linalg.norm(p - (v0 + t * (v1 - v0))))
    return best


N_PT, N_EYE, N_LT = 3600, 3000, 96
LAMP_RADIUS, LAMP_FOCUS = 0.08, 0.35


@pytest.fixture(scope="module")
def lamp(gpu, pkg):
    """scenes.lamp_floor(lamp_in_view=True) at 64 x 64 through a lens of radius 0.08 focused at 0.35 of the distance to the lookat point
    -- 1.6 in front of the eye, the lamp 4.5 away: by similar triangles (tests/test_camera_lens_cpu.py) a point of the lamp spreads over
    a disc of radius R (1 - focus / g) / (focus |U|) (w / 2) = 0.08 x 0.65 / (0.35 x 1.65) x 32 = 2.9 pixels, so the lamp's outline is
    blurred over about six.  Per-frame image and 8 x 8 block means of "pt" (with the lens and without), "SPCBPT_eye" and "lt"."""
    scene = pkg.scenes.lamp_floor(lamp_in_view=True)
    w = h = 64
    eye, U, V, Wv = (np.asarray(a, np.float64) for a in _frame(pkg, scene, w, h))
    tris = np.asarray(scene.vertices, np.float64)[np.asarray(scene.indices)]
    # every lens point keeps a margin to all geometry: the eye's distance to the nearest triangle, less the lens radius
    clearance = min(_point_triangle_distance(eye, t) for t in tris) - LAMP_RADIUS
    print(f"clearance of the lens disc to the nearest geometry: {clearance:.3f}")
    assert clearance > 0.5
    out = dict(scene=scene, w=w, h=h, frame=(eye, U, V, Wv), tris=tris)

    def eye_frames(r, alg, n):
        imgs = []
        for f in range(n):              # subframe f on a cleared film: accum = image / (f + 1)
            r.clear_accum()
            r.render_frame(alg, f)
            r.sync()
            imgs.append((f + 1) * r.read_accum()[..., :3].astype(np.float64))
        return np.array(imgs)

    def lt_frames(r, n):
        imgs = []
        for f in range(n):
            r.launch("light trace", f + 1)
            r.build_sampler()
            r.launch("lt", 0)
            r.sync()
            imgs.append(r.read_accum()[..., :3].astype(np.float64))
        return np.array(imgs)

    r = _renderer(pkg, scene, w, h, light=(20000, 16, 1), tuple_="minimal")
    out["pt pinhole"] = eye_frames(r, "pt", N_PT)
    r.set_lens(LAMP_RADIUS, LAMP_FOCUS)
    out["pt"] = eye_frames(r, "pt", N_PT)
    out["SPCBPT_eye"] = eye_frames(r, "SPCBPT_eye", N_EYE)
    rl = _renderer(pkg, scene, w, h, light=(200000, 8, 1), tuple_="minimal")
    rl.set_lens(LAMP_RADIUS, LAMP_FOCUS)
    out["lt"] = lt_frames(rl, N_LT)
    for k in ("pt pinhole", "pt", "SPCBPT_eye", "lt"):
        assert np.isfinite(out[k]).all(), k
    return out


def _blocks(imgs):
    n, h, w, _ = imgs.shape
    return _lum(imgs.reshape(n, h // 8, 8, w // 8, 8, 3).mean((2, 4)))


@pytest.mark.parametrize("alg", ["lt", "SPCBPT_eye"])
def test_three_estimators_agree_on_a_defocused_emitter(lamp, alg):
    """"lt" against "pt" and "SPCBPT_eye" against "pt" through the same lens: image means within 0.5 %, each image-mean standard error at
    most 0.005 / 3 of the mean (a condition, asserted), at least 99 % of the 8 x 8 blocks within 4 s + 0.5 % -- the bars of
    test_direct_light_against_quadrature.  And the comparison can fail: against the PINHOLE "pt" some blocks on the lamp's outline differ
    by more than 4 s, so a renderer that ignores the lens does not pass.  Frame counts from the measured per-frame spread ("pt" is the
    noisiest: 1.3e-3 of the mean after 3 600 frames of 64 x 64, a frame takes a quarter of a millisecond).  Measured on the MI355X:
    lt / pt = 0.99911, SPCBPT_eye / pt = 0.99981, 64 of 64 blocks inside for both, 33 / 32 blocks outside against the pinhole."""
    res = {}
    for k in (alg, "pt", "pt pinhole"):
        m = _lum(lamp[k].mean((1, 2)))
        res[k] = (m.mean(), m.std(ddof=1) / math.sqrt(len(m)))
        print(f"{k}: image mean {res[k][0]:.6f}, standard error {res[k][1] / res[k][0]:.2e} of it ({len(m)} frames)")
    base = res["pt"][0]
    for k in (alg, "pt"):
        assert res[k][1] <= 0.005 / 3 * base, (k, res[k][1], base)
    ratio = res[alg][0] / base
    ba, bp, b0 = _blocks(lamp[alg]), _blocks(lamp["pt"]), _blocks(lamp["pt pinhole"])
    s = np.sqrt(ba.var(0, ddof=1) / len(ba) + bp.var(0, ddof=1) / len(bp))
    diff = np.abs(ba.mean(0) - bp.mean(0))
    inside = diff <= 4 * s + 0.005 * bp.mean(0)
    z = (ba.mean(0) - bp.mean(0))[s > 0] / s[s > 0]
    print(f"{alg} / pt = {ratio:.5f}; 8 x 8 blocks inside 4 s + 0.5 %: {inside.mean():.4f}, z-scores mean {z.mean():+.2f} rms {np.sqrt((z * z).mean()):.2f} max |z| {np.abs(z).max():.2f}")
    s0 = np.sqrt(ba.var(0, ddof=1) / len(ba) + b0.var(0, ddof=1) / len(b0))
    off = np.abs(ba.mean(0) - b0.mean(0)) > 4 * s0 + 0.005 * b0.mean(0)
    print(f"against the pinhole pt: {int(off.sum())} of {off.size} blocks outside 4 s + 0.5 %")
    assert abs(ratio - 1) <= 0.005, ratio
    assert inside.mean() >= 0.99, (inside.mean(), np.abs(z).max())
    assert off.sum() >= 4, "the lens and the pinhole are indistinguishable: the comparison could not fail"


def test_deep_inside_and_far_outside(gpu, pkg):
    """A pixel whose whole cone -- its four corners crossed with 16 points on the lens rim -- lies on the lamp's front faces (the
    Moeller-Trumbore selection of test_a_seen_emitter_shows_its_radiance with its 1e-3 margins) shows Le within 4 standard errors + 0.5 %,
    for "pt" and for "lt": defocus averages radiance, it does not dim it (no cos^4, no aperture factor).  A pixel whose whole cone, and
    that of every pixel within three pixels of it, misses every triangle is exactly 0 in both.  At 128 x 128 with a lens of radius 0.04 focused at 0.35:
    the blur disc on the lamp has a radius of 2.9 pixels and 24 pixels lie wholly inside the lamp (at 64 x 64 the lamp is 23 x 10
    pixels and none does once the outline is blurred over several pixels)."""
    scene = pkg.scenes.lamp_floor(lamp_in_view=True)
    w = h = 128
    R, focus = 0.04, LAMP_FOCUS
    eye, U, V, Wv = (np.asarray(a, np.float64) for a in _frame(pkg, scene, w, h))
    tris = np.asarray(scene.vertices, np.float64)[np.asarray(scene.indices)]
    P64, _, _ = _light_geometry(pkg, scene)
    whole, empty = _cones(eye, U, V, Wv, w, h, R, focus, tris, P64)
    # (the cone test samples the pixel's corners and the lens rim: a triangle's image may reach into a pixel between those samples -- a
    # corner of the floor, or the outline as seen from a lens point between two rim samples, which lie up to 2.9 x 2 pi / 16 = 1.1
    # pixels apart -- so "far" keeps three pixels of distance to every pixel whose sampled cone touches anything)
    far = empty.copy()
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            sh = np.zeros_like(empty)
            sh[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] = empty[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
            far &= sh
    print(f"{int(whole.sum())} pixels wholly on the lamp's front faces, {int(far.sum())} far outside everything")
    assert whole.sum() >= 20 and far.sum() >= 1000
    Le = np.array(scene.mesh_lights[0]["emission"], np.float64)
    frames = {}
    r = _renderer(pkg, scene, w, h, light=(200000, 8, 1), tuple_="minimal")
    r.set_lens(R, focus)
    imgs = []
    for f in range(4):                  # every sample of such a pixel hits the lamp's front: "pt" adds exactly Le
        r.clear_accum()
        r.launch("pt", f)
        r.sync()
        imgs.append((f + 1) * r.read_accum()[..., :3].astype(np.float64))
    frames["pt"] = np.array(imgs)
    imgs = []
    for f in range(24):
        r.launch("light trace", f + 1)
        r.build_sampler()
        r.launch("lt", 0)
        r.sync()
        imgs.append(r.read_accum()[..., :3].astype(np.float64))
    frames["lt"] = np.array(imgs)
    for alg, imgs in frames.items():
        assert np.isfinite(imgs).all()
        per_frame = imgs[:, whole].mean(1)
        mean, se = per_frame.mean(0), per_frame.std(0, ddof=1) / math.sqrt(len(per_frame))
        print(f"{alg}: mean / Le = {mean / Le}, standard error / Le = {se / Le}")
        assert (np.abs(mean - Le) <= 4 * se + 0.005 * Le).all(), (alg, mean, Le, se)
        lit = (imgs != 0).any((0, 3))
        print(f"{alg}: far pixels that are not 0: {int((lit & far).sum())} (empty-cone pixels that are not 0: {int((lit & empty).sum())})")
        assert not (lit & far).any(), alg


# ------------------------------------------------------------------------------------------------------------ refusals
def test_forms_without_a_lens_kernel_refuse(gpu, pkg):
    """Every launch form that has no lens kernel returns SPCBPT_ERR_STATE with a message that names the lens and leaves the film
    untouched (hash of accum before and after); none renders a pinhole image silently.  With radius 0 the same calls go through."""
    scene = pkg.scenes.cornell_box()
    w, h = 48, 32
    r = _renderer(pkg, scene, w, h, light=(2000, 16, 1), tuple_="minimal")
    r.render_frame("SPCBPT_eye", 0)
    r.sync()
    R = _lens_of(pkg, scene, w, h)
    r.set_lens(R, 0.7)

    def digest():
        r.sync()
        return hashlib.sha256(r.read_accum().tobytes()).hexdigest()

    def refuses(fn, what):
        before = digest()
        with pytest.raises(pkg.SpcbptError) as e:
            fn()
        assert f"({STATE})" in str(e.value) and "lens" in str(e.value), (what, str(e.value))
        assert digest() == before, what

    refuses(lambda: r.launch_eye_batch([1]), "launch_eye_batch")
    refuses(lambda: r.launch_adaptive("SPCBPT_eye"), "launch_adaptive")
    refuses(lambda: r.launch("SPCBPT_no_rmis", 1), "SPCBPT_no_rmis")
    for mode in (1, 2):
        r.enable_counters(mode)
        refuses(lambda: r.launch("SPCBPT_eye", 1), f"SPCBPT_eye, counters {mode}")
        refuses(lambda: r.launch("pt", 1), f"pt, counters {mode}")
    r.enable_counters(0)
    # the forms that do have a lens kernel go through, deferred ones included
    for alg in ("SPCBPT_eye", "pt"):
        before = digest()
        r.launch_deferred(alg, 1)
        r.merge_deferred(True)
        assert digest() != before, alg
    r.launch("lt", 2)
    # ... and with the lens off again the refused forms render
    r.set_lens(0.0, 0.7)
    before = digest()
    r.launch("SPCBPT_no_rmis", 3)
    assert digest() != before
    # "SPCBPT_eye" under SPCBPT_ENV_EYE_SEES_SKY
    e = _renderer(pkg, scene, w, h, light=(2000, 16, 1), tuple_="minimal")
    e.set_environment(pkg.scenes.sky_texture())
    e.set_subspace()
    e.set_environment_mode(pkg.api.ENV_EYE_SEES_SKY)
    e.render_frame("SPCBPT_eye", 0)
    e.sync()
    e.set_lens(R, 0.7)
    before = hashlib.sha256(e.read_accum().tobytes()).hexdigest()
    with pytest.raises(pkg.SpcbptError) as err:
        e.launch("SPCBPT_eye", 1)
    assert f"({STATE})" in str(err.value) and "lens" in str(err.value), str(err.value)
    e.sync()
    assert hashlib.sha256(e.read_accum().tobytes()).hexdigest() == before
    e.set_environment_mode(0)
    e.launch("SPCBPT_eye", 1)      # without the sky strategy the lens form renders the scene with its environment map
    e.sync()
    assert np.isfinite(e.read_accum()).all()


# ------------------------------------------------------------------------------------------------------------ tool
def test_render_tool_takes_an_aperture(gpu, pkg, tmp_path):
    """tools/spcbpt_render --alg pt --emissive --aperture R --focus F on the lamp scene's glTF file, 64 x 64, 8 frames: the PFM's mean is
    the library's for the same eight subframes.  "pt" is a deterministic function of the seeds, but the tool's camera has been through
    the glTF file (a text round trip of its numbers): of the 32 768 samples a few next to the lamp's outline may fall on the other side
    of it, each moving the mean by up to Le / 32 768 / mean ~ 5e-4 of it -- the bar is 2e-3; and the same run without --aperture must
    NOT meet it on the lamp's pixels."""
    scene = pkg.scenes.lamp_floor(lamp_in_view=True)
    m = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "spcbpt_render"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert m.returncode == 0, m.stdout[-3000:]
    path = pkg.scenes.write_gltf(scene, str(tmp_path), "lamp")
    r = _renderer(pkg, scene, 64, 64, light=(20000, 16, 1))
    cam = scene.camera
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], 1.0)
    r.set_lens(LAMP_RADIUS, LAMP_FOCUS)
    for f in range(8):
        r.launch("pt", f)
    r.sync()
    want = r.read_accum()[..., :3].astype(np.float64)

    def tool(extra, name):
        out = os.path.join(str(tmp_path), name)
        cmd = [os.path.join(ROOT, "tools", "spcbpt_render"), path, ".", "--alg", "pt", "--emissive", "--dim=64x64", "--frames", "8", "--out", out] + extra
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-3000:]
        raw = open(out + ".pfm", "rb").read()
        head = raw.split(b"\n", 3)
        assert head[0] == b"PF" and head[1] == b"64 64"
        img = np.frombuffer(head[3], np.float32).reshape(64, 64, 3).astype(np.float64)
        assert np.isfinite(img).all()
        return p.stdout, img

    log, img = tool(["--aperture", str(LAMP_RADIUS), "--focus", str(LAMP_FOCUS)], "lens")
    assert "lens: radius 0.08, focus 0.35" in log, log
    _, sharp = tool([], "pinhole")
    got, ref, pin = _lum(img).mean(), _lum(want).mean(), _lum(sharp).mean()
    print(f"tool image mean {got:.6f} vs the library's {ref:.6f} (ratio {got / ref:.5f}); without --aperture {pin:.6f}")
    assert abs(got / ref - 1) <= 2e-3
    # the images themselves (the PFM's rows may run either way: compare the sorted pixel values): the lens blurs the lamp's outline,
    # so the sharp image holds many more pixels at the lamp's full radiance
    Le = sum(scene.mesh_lights[0]["emission"])
    full = lambda a: int((_lum(a) > 0.98 * Le).sum())
    print(f"pixels at the lamp's full radiance: tool {full(img)}, library {full(want)}, pinhole {full(sharp)}")
    assert abs(full(img) - full(want)) <= 2 and full(sharp) > full(img) + 20
