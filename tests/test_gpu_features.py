"""The first-hit feature pass (spcbpt_launch_features): albedo + coverage and normal + depth of what the film's primary ray sees first,
against a float64 recomputation from the scene's own arrays.  The hit itself (triangle, distance, barycentrics) comes from the
existing stand-alone traversal entry point, Renderer.trace_closest, on float64 pixel-centre rays rounded to float32; everything after
the hit -- the normal from the triangle's corners, the face-forwarding, the bilinear + wrap + pow 2.2 texture fetch, the emitter and
miss rules -- is recomputed here.

Bars, each a few float32 ulp through the operation named: normal 2e-6 absolute (a normalised cross product of float32 corners),
depth 1e-5 relative (the device's own ray differs from the rounded float64 one in the last bit), untextured albedo equal to
float32(colour), textured albedo 5e-4 absolute (one ulp of (u, v) x 64 texels x checker contrast, through pow 2.2), coverage
exactly 0 or 1.  A pixel is left out only if five host rays -- the centre and its four offsets of 1e-3 pixel -- disagree on the
triangle: at most 2 % of the pixels.

Measured on the MI355X (largest deviations): see DESIGN.md 8c."""
import numpy as np
import pytest

from tests.test_gpu_mesh_light import _renderer

pytestmark = pytest.mark.gpu

STATE, INVALID = -5, -1


# ------------------------------------------------------------------------------------------------------------ truth
def _camera(pkg, scene, w, h):
    cam = scene.camera
    U, V, W = pkg.camera_frame(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
    return np.array(cam["eye"], np.float32), U, V, W


def _rays(eye, U, V, W, w, h, ox=0.0, oy=0.0):
    """float64 rays through pixel centre + (ox, oy) pixels, rounded to float32, in trace_closest's layout; and the float64 directions."""
    y, x = np.mgrid[0:h, 0:w]
    dx = 2.0 * ((x + 0.5 + ox) / w) - 1.0
    dy = 2.0 * ((y + 0.5 + oy) / h) - 1.0
    d = dx[..., None] * U.astype(np.float64) + dy[..., None] * V.astype(np.float64) + W.astype(np.float64)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    rays = np.zeros((h * w, 8), np.float32)
    rays[:, 0:3] = eye
    rays[:, 3] = 1e-3        # SPCBPT_SCENE_EPSILON
    rays[:, 4:7] = d.reshape(-1, 3)
    rays[:, 7] = 1e16
    return rays, d.reshape(-1, 3)


def _texture64(tex, u, v):
    """bilinear + wrap fetch of an (h, w, 4) uint8 texture at (u, v) in float64 (tex_fetch_rgb), then pow 2.2."""
    th, tw = tex.shape[:2]
    x, y = u * tw - 0.5, v * th - 0.5
    fx, fy = np.floor(x), np.floor(y)
    ax, ay = x - fx, y - fy
    x0, y0 = fx.astype(np.int64) % tw, fy.astype(np.int64) % th
    x1, y1 = (x0 + 1) % tw, (y0 + 1) % th
    t = tex[..., :3].astype(np.float64) / 255.0
    c = (((1 - ax) * (1 - ay))[:, None] * t[y0, x0] + (ax * (1 - ay))[:, None] * t[y0, x1]
         + ((1 - ax) * ay)[:, None] * t[y1, x0] + (ax * ay)[:, None] * t[y1, x1])
    return c ** 2.2


def feature_truth(scene, tracer, eye, U, V, W, w, h):
    """-> albedo (h, w, 4), normal_depth (h, w, 4) in float64, textured (h, w) bool, excluded (h, w) bool, tri (h, w).
    `tracer(rays) -> (t, tri, uv)` is Renderer.trace_closest."""
    rays, d = _rays(eye, U, V, W, w, h)
    t, tri, uv = tracer(rays)
    excluded = np.zeros(h * w, bool)
    for ox, oy in ((1e-3, 0), (-1e-3, 0), (0, 1e-3), (0, -1e-3)):
        _, tri_o, _ = tracer(_rays(eye, U, V, W, w, h, ox, oy)[0])
        excluded |= tri_o != tri
    P = np.asarray(scene.vertices, np.float32).astype(np.float64)
    I = np.asarray(scene.indices, np.int64)
    nt = len(I)
    albedo = np.zeros((h * w, 4))
    albedo[:, :3] = 1.0
    nd = np.zeros((h * w, 4))
    textured = np.zeros(h * w, bool)
    surf = np.nonzero((tri >= 0) & (tri < nt))[0]
    c = P[I[tri[surf]]]
    n = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n[(n * d[surf]).sum(1) > 0] *= -1.0
    nd[surf, :3], nd[surf, 3] = n, t[surf].astype(np.float64)
    albedo[surf, 3] = 1.0
    mat = np.asarray(scene.tri_material)[tri[surf]]
    for m in np.unique(mat):
        sel = surf[mat == m]
        md = scene.materials[int(m)]
        if md.get("albedo_tex", 0) > 0:
            T = np.asarray(scene.texcoords, np.float32).astype(np.float64)[I[tri[sel]]]
            bu, bv = uv[sel, 0].astype(np.float64), uv[sel, 1].astype(np.float64)
            st = (1 - bu - bv)[:, None] * T[:, 0] + bu[:, None] * T[:, 1] + bv[:, None] * T[:, 2]
            albedo[sel, :3] = _texture64(np.asarray(scene.textures[md["albedo_tex"] - 1]), st[:, 0], st[:, 1])
            textured[sel] = True
        else:
            albedo[sel, :3] = np.asarray(md.get("color", (1, 1, 1)), np.float32).astype(np.float64)
    emit = np.nonzero(tri >= nt)[0]
    for i in emit:   # a quad light's two triangles follow the scene's; back faces never get here (culled in the traversal), the rule is kept
        L = scene.lights[(tri[i] - nt) // 2]
        ln = np.cross(np.asarray(L["u"], np.float32).astype(np.float64), np.asarray(L["v"], np.float32).astype(np.float64))
        ln /= np.linalg.norm(ln)
        if d[i] @ ln > 0:
            continue
        albedo[i, 3] = 1.0
        nd[i, :3], nd[i, 3] = ln, float(t[i])
    shape = lambda a: a.reshape((h, w) + a.shape[1:])
    return shape(albedo), shape(nd), shape(textured), shape(excluded), shape(tri)


def check_features(scene, r, pkg, w, h, name):
    eye, U, V, W = _camera(pkg, scene, w, h)
    alb_t, nd_t, textured, excluded, tri = feature_truth(scene, r.trace_closest, eye, U, V, W, w, h)
    r.launch_features(0)
    alb, nd = r.read_features()
    ok = ~excluded
    nt = len(scene.indices)
    hit = tri >= 0
    print(f"{name} {w}x{h}: excluded {excluded.mean():.4f}; surface {((tri >= 0) & (tri < nt)).mean():.3f}, emitter {(tri >= nt).mean():.4f}, "
          f"miss {(~hit).mean():.3f}, textured {textured.mean():.3f}")
    assert excluded.mean() <= 0.02
    assert np.isin(alb[..., 3], (0.0, 1.0)).all()
    assert np.array_equal(alb[..., 3][ok], alb_t[..., 3][ok])
    dn = np.abs(nd[..., :3].astype(np.float64) - nd_t[..., :3])[ok].max()
    sel = ok & hit
    dd = (np.abs(nd[..., 3].astype(np.float64) - nd_t[..., 3])[sel] / nd_t[..., 3][sel]).max()
    plain = ok & ~textured
    da = np.abs(alb[..., :3].astype(np.float64) - alb_t[..., :3])[ok & textured].max() if (ok & textured).any() else 0.0
    print(f"  largest deviations: normal {dn:.3g}, depth {dd:.3g} relative, textured albedo {da:.3g}")
    assert dn <= 2e-6
    assert dd <= 1e-5
    assert np.array_equal(alb[..., :3][plain], alb_t[..., :3][plain].astype(np.float32))
    assert da <= 5e-4
    miss = ok & ~hit
    assert (nd[miss] == 0).all() and (alb[miss] == np.float32([1, 1, 1, 0])).all()
    return alb, nd, tri, excluded


# ------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("w,h", [(48, 32), (43, 29)])
def test_cornell_first_hit(gpu, pkg, w, h):
    scene = pkg.scenes.cornell_box()
    r = _renderer(pkg, scene, w, h)
    alb, _, tri, _ = check_features(scene, r, pkg, w, h, "cornell")
    assert 0.3 < alb[..., 3].mean() < 0.5          # the box fills about 37 % of this view; the rest is a miss


@pytest.fixture(scope="module")
def bedroom(gpu, pkg):
    return pkg.scenes.bedroom(target_tris=20_000, tex_size=64)


def test_bedroom_textures_and_emitter(gpu, pkg, bedroom):
    w, h = 48, 32
    r = _renderer(pkg, bedroom, w, h)
    alb, _, tri, excluded = check_features(bedroom, r, pkg, w, h, "bedroom")
    mats = np.asarray(bedroom.tri_material)
    nt = len(bedroom.indices)
    on_tex = [bedroom.materials[int(mats[t])].get("albedo_tex", 0) > 0 for t in tri[(tri >= 0) & (tri < nt)]]
    assert sum(on_tex) > 100, "textured surfaces in view"
    assert (tri >= nt).any(), "an emitter in view"


def test_bands(gpu, pkg):
    """Rows outside the band set are untouched, and two disjoint band sets together equal the full launch bit for bit."""
    scene = pkg.scenes.cornell_box()
    w, h = 48, 32
    r = _renderer(pkg, scene, w, h)
    r.launch_features(0)
    full = [a.copy() for a in r.read_features()]
    r.launch_features(1, (0, 16, 1))              # subframe 1 jitters: the launch's rows move, the others must not
    a = [x.copy() for x in r.read_features()]
    for x, f in zip(a, full):
        assert x[16:].tobytes() == f[16:].tobytes()
    assert not np.array_equal(a[1][:16], full[1][:16])
    r.resize(w, h)                                 # fresh (zeroed) buffers
    r.launch_features(0, (0, 16, 1))
    a = [x.copy() for x in r.read_features()]
    for x, f in zip(a, full):
        assert x[:16].tobytes() == f[:16].tobytes() and not x[16:].any()
    r.launch_features(0, (16, h, 1))
    for x, f in zip(r.read_features(), full):
        assert x.tobytes() == f.tobytes()
    r.resize(w, h)
    r.launch_features(0, (0, h, 2))                # bands 0 and 2
    for x, f in zip(r.read_features(), full):
        for band in (0, 2):
            assert x[8 * band:8 * band + 8].tobytes() == f[8 * band:8 * band + 8].tobytes()
        for band in (1, 3):
            assert not x[8 * band:8 * band + 8].any()
    with pytest.raises(pkg.SpcbptError, match=rf"\({INVALID}\)"):
        r.launch_features(0, (4, h, 1))


def test_running_mean_over_subframes(gpu, pkg):
    """Subframes 0..7: coverage stays in [0, 1], the mean normal is no longer than 1, and a pixel whose 3 x 3 neighbourhood saw one
    triangle at subframe 0 -- its whole footprint lies on that triangle -- keeps the triangle's normal."""
    scene = pkg.scenes.cornell_box()
    w, h = 48, 32
    r = _renderer(pkg, scene, w, h)
    eye, U, V, W = _camera(pkg, scene, w, h)
    _, nd_t, _, _, tri = feature_truth(scene, r.trace_closest, eye, U, V, W, w, h)
    for f in range(8):
        r.launch_features(f)
    alb, nd = r.read_features()
    assert np.isfinite(alb).all() and np.isfinite(nd).all()
    assert (alb[..., 3] >= 0).all() and (alb[..., 3] <= 1).all()
    assert (np.linalg.norm(nd[..., :3].astype(np.float64), axis=-1) <= 1 + 1e-6).all()
    same = np.zeros((h, w), bool)
    same[1:-1, 1:-1] = tri[1:-1, 1:-1] >= 0
    for oy in (-1, 0, 1):
        for ox in (-1, 0, 1):
            same[1:-1, 1:-1] &= tri[1 + oy:h - 1 + oy, 1 + ox:w - 1 + ox] == tri[1:-1, 1:-1]
    print(f"{int(same.sum())} of {w * h} pixels lie wholly on one triangle")
    assert same.sum() > 50
    assert np.abs(nd[..., :3].astype(np.float64) - nd_t[..., :3])[same].max() <= 1e-6
    assert (alb[..., 3][same] == 1).all()
    assert (nd[..., 3][same] > 0).all()


def test_the_film_is_not_touched(gpu, pkg):
    scene = pkg.scenes.cornell_box()
    w, h = 48, 32
    r = _renderer(pkg, scene, w, h)
    for f in range(2):
        r.launch("pt", f)
    accum, frame = r.read_accum().copy(), r.read_frame().copy()
    r.launch_features(0)
    r.launch_features(1)
    r.sync()
    assert r.read_accum().tobytes() == accum.tobytes() and r.read_frame().tobytes() == frame.tobytes()
    r.launch("pt", 2)                               # ... and the film goes on where it was
    r.sync()
    assert np.isfinite(r.read_accum()).all()


def test_errors_leave_the_context_usable(gpu, pkg):
    scene = pkg.scenes.cornell_box()
    w, h = 48, 32
    cam = scene.camera

    def fails(fn, code, text=None):
        with pytest.raises(pkg.SpcbptError) as e:
            fn()
        assert f"({code})" in str(e.value), str(e.value)
        if text:
            assert text in str(e.value), str(e.value)

    r = pkg.Renderer(scene, 0)
    fails(lambda: r.launch_features(0), STATE, "resize")                      # no film
    r.resize(w, h)
    fails(lambda: r.launch_features(0), STATE, "camera")                      # no camera
    U, V, W = pkg.camera_frame(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
    r.set_camera(np.array(cam["eye"], np.float32), U, V, W)
    fails(lambda: r.read_features(), STATE, "no feature launch")              # nothing rendered yet
    r.launch_deferred("pt", 0)
    fails(lambda: r.launch_features(0), STATE, "deferred")                    # a deferred frame outstanding
    r.merge_deferred(True)
    r.launch_features(0)
    alb, nd = r.read_features()
    assert alb[..., 3].max() == 1 and nd[..., 3].max() > 0
    r.resize(w, h)
    fails(lambda: r.read_features(), STATE)                                   # ... and a resize forgets them
    r.launch_features(0)
    assert np.array_equal(r.read_features()[0], alb)
