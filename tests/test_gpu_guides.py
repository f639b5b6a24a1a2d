"""The reflected guide planes (spcbpt_launch_guides) and the switch that makes denoise / denoise_variance read them.

1. The planes against the float64 chain of tests/guides_ref.py (all-triangles caster, nothing of the product in it) on scenes.mirror_box()
   at max_bounces 1, 2 and 4, at 44 x 28 (partial tiles), and on the bedroom with the defaults.  A pixel is left out only if the float64
   chains through its centre and through its four offsets of 1e-3 pixel disagree on the triangle sequence: at most 5 % (mirror_box
   0.07 %, bedroom 1.2 %, counted on the CPU with guides_ref alone).  On the others coverage is exact and, per number of mirrors followed,
       normal 2e-6 absolute, depth 1e-5 relative, textured albedo 5e-4 absolute      (tests/test_gpu_features.py's bars, not widened),
       untextured albedo: float32(colour) exactly with no mirror; behind mirrors 2e-6 absolute -- the product of up to 8 tints, each
       within 4 float32 ulp of its definition (tests/test_guide_step_cpu.py) and 5 x 1e-7 from the fifth power's slope at the last bit of |N.d|.
   The arms: mirror_box at max_bounces >= 2 ends at least 20 pixels on each of mirror -> surface, mirror -> mirror -> surface,
   mirror -> emitter and mirror -> miss (389 / 82 / 28 / 189 of 1536); with max_bounces = 1 the second mirror is a surface by definition,
   so the two-mirror arm is asserted empty there.  The bedroom is a closed room with four small mirror spheres: its 48 x 32 view has
   mirror -> surface (156 pixels) and a handful of mirror -> emitter (6), no second mirror and no way out; the test asserts the arm it has.
2. max_bounces = 0 and roughness_max = -1 give read_features() bit for bit (subframes 0 and 3).
3. Bands, partial tiles, the running mean.   4. Nothing else moves.
5. The point of it: an 8-frame "pt" film of mirror_box denoised with either pair of guides against a 512-frame film, over the pixels
   whose first hit is a mirror: the reflected guides' RMSE must be the lower one.
   The two denoised images can be equal bit for bit only where the filter saw no mirror pixel: the a-trous taps of iteration i reach
   2 x 2^i pixels, so a pixel next to a mirror weighs mirror pixels, whose guides and demodulated colours differ between the two pairs.
   The check is therefore made where it can hold: the guide planes equal the feature planes bit for bit on every pixel whose first hit is
   not a mirror, and with 1 and 2 iterations (reach 2 and 6 pixels) the two denoised images are equal bit for bit on every pixel
   farther than that from all mirror pixels.  At the default 5 iterations the reach (62) is the whole 48 x 32 image.
6. Refusals leave the context usable.

Measured on the MI355X, largest deviations per number of mirrors followed (normal / depth relative / textured albedo / untextured albedo);
no bar had to grow beyond its start:
    mirror_box, max_bounces 4   0 mirrors 1.9e-8 / 3.2e-7 / 1.5e-5 / exact;  1 mirror 3.5e-8 / 3.9e-7 / 1.5e-5 / 5.0e-8;  2 mirrors 1.9e-8 / 5.0e-7 / 4.0e-6 / 7.3e-8
    mirror_box, max_bounces 1   1 mirror 3.5e-8 / 3.9e-7 / 1.5e-5 / 5.3e-8          44 x 28: 2 mirrors 1.9e-8 / 2.2e-7 / 9.2e-6 / 7.1e-8
    bedroom                     0 mirrors 1.3e-7 / 2.5e-6 / 4.6e-5 / exact;  1 mirror 3.9e-7 / 7.5e-7 / 1.8e-5 / 5.0e-8
RMSE over the 689 mirror pixels of mirror_box, 8 frames against 512: film 0.776, first-hit guides 0.671, reflected guides 0.619 (ratio 0.92);
736 of the 847 other pixels differ between the two results at 5 iterations.  """
import numpy as np
import pytest

from tests import guides_ref as gr
from tests.test_gpu_mesh_light import _renderer

pytestmark = pytest.mark.gpu

STATE, INVALID = -5, -1
W_, H_ = 48, 32
BAR_NORMAL, BAR_DEPTH, BAR_TEX, BAR_PLAIN = 2e-6, 1e-5, 5e-4, 2e-6


def _camera(pkg, scene, w, h):
    cam = scene.camera
    U, V, W = pkg.camera_frame(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
    return np.array(cam["eye"], np.float32), U, V, W


@pytest.fixture(scope="module")
def box(pkg):
    return pkg.scenes.mirror_box()


_truths = {}


def _truth(pkg, scene, w, h, **kw):
    key = (scene.name, w, h, tuple(sorted(kw.items())))
    if key not in _truths:
        _truths[key] = gr.guide_truth(scene, *_camera(pkg, scene, w, h), w, h, **kw)
    return _truths[key]


def _check(pkg, scene, r, w, h, name, **kw):
    c = _truth(pkg, scene, w, h, **kw)
    r.launch_guides(0, **kw)
    alb, nd = r.read_guides()
    ok = ~c["excluded"]
    arms = gr.arms(c)
    print(f"{name} {w}x{h} {kw}: excluded {c['excluded'].mean():.4f}; arms {arms}")
    assert c["excluded"].mean() <= 0.05
    assert np.isin(alb[..., 3], (0.0, 1.0)).all()
    assert np.array_equal(alb[..., 3][ok], c["albedo"][..., 3][ok])
    alb_t, nd_t = c["albedo"], c["normal_depth"]
    for b in range(int(c["bounces"].max()) + 1):
        sel = ok & (c["bounces"] == b)
        if not sel.any():
            continue
        dn = np.abs(nd[..., :3].astype(np.float64) - nd_t[..., :3])[sel].max()
        far = sel & (nd_t[..., 3] > 0)
        dd = (np.abs(nd[..., 3].astype(np.float64) - nd_t[..., 3])[far] / nd_t[..., 3][far]).max() if far.any() else 0.0
        tex, plain = sel & c["textured"], sel & ~c["textured"]
        dt = np.abs(alb[..., :3].astype(np.float64) - alb_t[..., :3])[tex].max() if tex.any() else 0.0
        dp = np.abs(alb[..., :3].astype(np.float64) - alb_t[..., :3])[plain].max() if plain.any() else 0.0
        print(f"  {b} mirrors, {int(sel.sum())} pixels: normal {dn:.3g}, depth {dd:.3g} relative, textured albedo {dt:.3g}, untextured albedo {dp:.3g}")
        assert dn <= BAR_NORMAL
        assert dd <= BAR_DEPTH
        assert dt <= BAR_TEX
        if b == 0:
            assert np.array_equal(alb[..., :3][plain], alb_t[..., :3][plain].astype(np.float32))
        else:
            assert dp <= BAR_PLAIN
    miss = ok & (c["end"] == gr.END_MISS0)
    assert (nd[miss] == 0).all() and (alb[miss] == np.float32([1, 1, 1, 0])).all()
    return c, arms


# ------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("max_bounces", [1, 2, 4])
def test_chain_against_float64_mirror_box(gpu, pkg, box, max_bounces):
    r = _renderer(pkg, box, W_, H_)
    c, arms = _check(pkg, box, r, W_, H_, "mirror_box", max_bounces=max_bounces)
    assert arms["mirror_surface"] >= 20 and arms["mirror_emitter"] >= 20 and arms["mirror_miss"] >= 20
    if max_bounces >= 2:
        assert arms["mirror_mirror_surface"] >= 20
    else:
        assert arms["mirror_mirror_surface"] == 0 and c["bounces"].max() == 1


def test_chain_against_float64_bedroom(gpu, pkg):
    scene = pkg.scenes.bedroom(target_tris=20_000, tex_size=64)
    r = _renderer(pkg, scene, W_, H_)
    c, arms = _check(pkg, scene, r, W_, H_, "bedroom")
    assert arms["mirror_surface"] >= 20
    assert (c["textured"] & (c["bounces"] == 0)).sum() > 100


# ------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("kw", [dict(max_bounces=0), dict(roughness_max=-1.0)])
def test_no_mirror_followed_is_the_first_hit(gpu, pkg, box, kw):
    r = _renderer(pkg, box, W_, H_)
    for f in (0, 3):
        r.resize(W_, H_)
        for k in range(f + 1):
            r.launch_features(k)
            r.launch_guides(k, **kw)
        for a, b in zip(r.read_guides(), r.read_features()):
            assert a.tobytes() == b.tobytes()
    r.launch_guides(4)                                   # ... and the defaults do differ on this scene
    assert r.read_guides()[0].tobytes() != r.read_features()[0].tobytes()


# ------------------------------------------------------------------------------------------------------------ 3
def test_bands(gpu, pkg, box):
    w, h = W_, H_
    r = _renderer(pkg, box, w, h)
    r.launch_guides(0)
    full = [a.copy() for a in r.read_guides()]
    r.launch_guides(1, (0, 16, 1))                       # subframe 1 jitters: the launch's rows move, the others must not
    a = [x.copy() for x in r.read_guides()]
    for x, f in zip(a, full):
        assert x[16:].tobytes() == f[16:].tobytes()
    assert not np.array_equal(a[1][:16], full[1][:16])
    r.resize(w, h)                                       # fresh (zeroed) planes
    r.launch_guides(0, (0, 16, 1))
    for x, f in zip(r.read_guides(), full):
        assert x[:16].tobytes() == f[:16].tobytes() and not x[16:].any()
    r.launch_guides(0, (16, h, 1))
    for x, f in zip(r.read_guides(), full):
        assert x.tobytes() == f.tobytes()
    r.resize(w, h)
    r.launch_guides(0, (0, h, 2))                        # bands 0 and 2 ...
    for x, f in zip(r.read_guides(), full):
        for band in (1, 3):
            assert not x[8 * band:8 * band + 8].any()
    r.launch_guides(0, (8, h, 2))                        # ... and 1 and 3: together the full launch
    for x, f in zip(r.read_guides(), full):
        assert x.tobytes() == f.tobytes()


def test_partial_tiles(gpu, pkg, box):
    r = _renderer(pkg, box, 44, 28)
    _check(pkg, box, r, 44, 28, "mirror_box", max_bounces=4)


def test_running_mean_over_subframes(gpu, pkg, box):
    r = _renderer(pkg, box, W_, H_)
    for f in range(8):
        r.launch_guides(f)
    alb, nd = r.read_guides()
    assert np.isfinite(alb).all() and np.isfinite(nd).all()
    assert (alb[..., 3] >= 0).all() and (alb[..., 3] <= 1).all()
    assert (np.linalg.norm(nd[..., :3].astype(np.float64), axis=-1) <= 1 + 1e-6).all()
    assert (nd[..., 3] >= 0).all()


# ------------------------------------------------------------------------------------------------------------ 4
def test_nothing_else_moves(gpu, pkg, box):
    r = _renderer(pkg, box, W_, H_)
    r.set_film_moments(True)
    r.set_film_buckets(4)
    for f in range(3):
        r.launch("pt", f)
        r.launch_features(f)
    r.denoise()
    dn = r.read_denoised()[0].copy()
    r.denoise_variance()
    dv = r.read_denoised()[0].copy()
    before = [r.read_accum().copy(), r.read_frame().copy(), *[a.copy() for a in r.read_features()], r.read_film_moments().copy(), r.read_film_buckets().copy()]
    for f in range(3):
        r.launch_guides(f)
    r.sync()
    after = [r.read_accum(), r.read_frame(), *r.read_features(), r.read_film_moments(), r.read_film_buckets()]
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    r.denoise()                                          # the switch at its default: the bits from before any guide launch
    assert r.read_denoised()[0].tobytes() == dn.tobytes()
    r.denoise_variance()
    assert r.read_denoised()[0].tobytes() == dv.tobytes()
    r.set_denoise_guides("reflected")                    # ... and the switch does something, and goes back
    r.denoise()
    assert r.read_denoised()[0].tobytes() != dn.tobytes()
    r.denoise_variance()
    assert r.read_denoised()[0].tobytes() != dv.tobytes()
    r.set_denoise_guides("first_hit")
    r.denoise()
    assert r.read_denoised()[0].tobytes() == dn.tobytes()
    r.launch("pt", 3)                                    # the film goes on where it was
    r.sync()
    assert np.isfinite(r.read_accum()).all()


# ------------------------------------------------------------------------------------------------------------ 5
def _reach(mask, k):
    """pixels within Chebyshev distance k of a pixel of `mask`"""
    out = mask.copy()
    h, w = mask.shape
    ys, xs = np.nonzero(mask)
    for y, x in zip(ys, xs):
        out[max(0, y - k):y + k + 1, max(0, x - k):x + k + 1] = True
    return out


def test_reflected_guides_denoise_the_mirror_better(gpu, pkg, box):
    w, h = W_, H_
    mirror = _truth(pkg, box, w, h, max_bounces=4)["first"]
    assert mirror.sum() > 400
    ref = _renderer(pkg, box, w, h)
    for f in range(512):
        ref.launch("pt", f)
    truth = ref.read_accum()[..., :3].astype(np.float64)
    r = _renderer(pkg, box, w, h)
    for f in range(8):
        r.launch("pt", f)
        r.launch_features(f)
        r.launch_guides(f)
    fa, fn = r.read_features()
    ga, gn = r.read_guides()
    # (the jittered subframes may put a pixel's samples on either side of a mirror's edge: "not a mirror" is taken over a 1-pixel margin)
    off = ~_reach(mirror, 1)
    assert fa[off].tobytes() == ga[off].tobytes() and fn[off].tobytes() == gn[off].tobytes()
    out = {}
    for which in ("first_hit", "reflected"):
        r.set_denoise_guides(which)
        r.denoise()
        out[which] = r.read_denoised()[0][..., :3].astype(np.float64)
    rmse = {k: float(np.sqrt(((v - truth) ** 2)[mirror].mean())) for k, v in out.items()}
    noisy = float(np.sqrt(((r.read_accum()[..., :3].astype(np.float64) - truth) ** 2)[mirror].mean()))
    changed = int((out["first_hit"] != out["reflected"]).any(-1)[~mirror].sum())
    print(f"RMSE over the {int(mirror.sum())} mirror pixels: 8-frame film {noisy:.4g}, first-hit guides {rmse['first_hit']:.4g}, reflected guides {rmse['reflected']:.4g}, "
          f"ratio {rmse['reflected'] / rmse['first_hit']:.3f}; {changed} of {int((~mirror).sum())} other pixels differ at 5 iterations (reach 62 pixels)")
    assert rmse["reflected"] < rmse["first_hit"]
    for iterations, reach in ((1, 2), (2, 6)):
        res = []
        for which in ("first_hit", "reflected"):
            r.set_denoise_guides(which)
            r.denoise(iterations=iterations)
            res.append(r.read_denoised()[0].copy())
        far = ~_reach(mirror, reach + 1)
        assert far.sum() > 100
        assert res[0][far].tobytes() == res[1][far].tobytes()
        assert res[0][mirror].tobytes() != res[1][mirror].tobytes()


# ------------------------------------------------------------------------------------------------------------ 6
def test_refusals_leave_the_context_usable(gpu, pkg, box):
    w, h = W_, H_
    cam = box.camera

    def fails(fn, code, text=None):
        with pytest.raises(pkg.SpcbptError) as e:
            fn()
        assert f"({code})" in str(e.value), str(e.value)
        if text:
            assert text in str(e.value), str(e.value)

    def works(r):
        r.launch_guides(0)
        alb, nd = r.read_guides()
        assert alb[..., 3].max() == 1 and nd[..., 3].max() > 0

    r = pkg.Renderer(box, 0)
    fails(lambda: r.launch_guides(0), STATE, "resize")
    r.resize(w, h)
    fails(lambda: r.launch_guides(0), STATE, "camera")
    U, V, W = pkg.camera_frame(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
    r.set_camera(np.array(cam["eye"], np.float32), U, V, W)
    fails(lambda: r.read_guides(), STATE, "no guide launch")
    r.set_light_trace(20000, 16, 1)
    r.launch("pt", 0)
    r.launch_features(0)
    r.set_film_moments(True)
    r.set_denoise_guides("reflected")
    fails(lambda: r.denoise(), STATE, "spcbpt_launch_guides")
    fails(lambda: r.denoise_variance(), STATE, "spcbpt_launch_guides")
    works(r)
    r.denoise()
    r.denoise_variance()
    assert np.isfinite(r.read_denoised()[0]).all()
    for kw in (dict(max_bounces=-1), dict(max_bounces=9), dict(roughness_max=float("nan")), dict(metallic_min=float("nan"))):
        fails(lambda: r.launch_guides(0, **kw), INVALID)
        works(r)
    fails(lambda: r.launch_guides(0, (4, h, 1)), INVALID, "row_begin")
    works(r)
    fails(lambda: r.set_denoise_guides(2), INVALID)
    works(r)
    r.launch_deferred("pt", 1)
    fails(lambda: r.launch_guides(1), STATE, "deferred")
    r.merge_deferred(True)
    works(r)
    r.resize(w, h)                                        # a resize forgets the planes, not the switch
    fails(lambda: r.read_guides(), STATE)
    r.launch("pt", 0)
    r.launch_features(0)
    fails(lambda: r.denoise(), STATE, "spcbpt_launch_guides")
    works(r)
    r.denoise()
