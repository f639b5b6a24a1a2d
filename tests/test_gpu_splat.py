"""The light-tracing estimator "lt" (spcbpt_launch(ctx, "lt", ...)): every vertex of the light-vertex cache connected straight to the
camera and splatted onto the film.  Checked against a float64 recount of the cache it read, against direct-light quadrature, against
the emitter's radiance and against "pt" -- an estimator it shares no camera-side code with."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_mesh_light import _direct_light, _light_geometry, _lum, _renderer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.float32(1e-3)   # SPCBPT_SCENE_EPSILON


# ------------------------------------------------------------------------------------------------------------ helpers
def _frame(pkg, scene, w, h):
    cam = scene.camera
    U, V, W = pkg.camera_frame(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
    return np.array(cam["eye"], np.float32), U, V, W


def _project64(eye, U, V, W, w, h, p):
    """float64 projection of points p (n, 3): continuous pixel coordinates (fx, fy), depth g, and the importance We."""
    eye, U, V, W = (np.asarray(a, np.float64) for a in (eye, U, V, W))
    c = np.asarray(p, np.float64) - eye
    D = U @ np.cross(V, W)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = c @ np.cross(U, V) / D
        dx = (c @ np.cross(V, W) / D) / g
        dy = (c @ np.cross(W, U) / D) / g
        we = w * h * np.linalg.norm(c / g[:, None], axis=1) ** 3 / (4 * abs(D))
    return (dx + 1) / 2 * w, (dy + 1) / 2 * h, g, we


def _shadow_rays(eye, pos):
    """The rays k_lt_splat shoots, operation for operation in float32: from the vertex towards the eye, (kEps, |c| - kEps)."""
    f = np.float32
    bias = (eye.astype(f)[None, :] - pos.astype(f)).astype(f)
    r2 = ((bias[:, 0] * bias[:, 0]).astype(f) + (bias[:, 1] * bias[:, 1]).astype(f)).astype(f)
    r2 = (r2 + (bias[:, 2] * bias[:, 2]).astype(f)).astype(f)
    ln = np.sqrt(r2, dtype=f)
    inv = (f(1.0) / ln).astype(f)
    d = (bias * inv[:, None]).astype(f)
    rays = np.zeros((len(pos), 8), f)
    rays[:, 0:3] = pos
    rays[:, 3] = EPS
    rays[:, 4:7] = d
    rays[:, 7] = (ln - EPS).astype(f)
    return rays


def _host_film(pkg, ob, r, scene, v, path_count, w, h, edge=1e-4, graze=1e-3):
    """The film "lt" must have written for cache `v`, recomputed in float64 -> (film (h, w, 3), excluded (h, w) bool, lit (h, w) bool,
    survivors, vertices).  `excluded` marks the pixels whose value hangs on a float32 decision: a vertex projects within `edge` pixel of
    a pixel edge (both pixels along that edge: the device may land it next door; float32 pixel coordinates are good to ~2.4e-5 pixel
    at 48 pixels, `edge` is four times that) or sees the eye at a grazing angle below `graze` (the back-face test may go either way)."""
    eye, U, V, W = _frame(pkg, scene, w, h)
    pos = np.asarray(v["position"], np.float32).reshape(-1, 3)
    nrm = np.asarray(v["normal"], np.float64).reshape(-1, 3)
    flux = np.asarray(v["flux"], np.float64).reshape(-1, 3)
    fx, fy, g, we = _project64(eye, U, V, W, w, h, pos)
    c = pos.astype(np.float64) - eye.astype(np.float64)
    r2 = (c * c).sum(1)
    to_cam = -c / np.sqrt(r2)[:, None]
    cosb = (nrm * to_cam).sum(1)
    excluded = np.zeros((h, w), bool)
    front = g > 0
    near = front & (fx > -edge) & (fx < w + edge) & (fy > -edge) & (fy < h + edge) & (flux.sum(1) > 0)

    def touch(mask, spread):
        for i in np.nonzero(mask)[0]:
            xs = {int(math.floor(fx[i] + s * spread)) for s in (-1, 0, 1)}
            ys = {int(math.floor(fy[i] + s * spread)) for s in (-1, 0, 1)}
            for y in ys:
                for x in xs:
                    if 0 <= x < w and 0 <= y < h:
                        excluded[y, x] = True
    on_edge = near & ((np.abs(fx - np.round(fx)) < edge) | (np.abs(fy - np.round(fy)) < edge))
    touch(on_edge, edge)
    touch(near & (np.abs(cosb) < graze), 0.0)
    inside = front & (fx >= 0) & (fx < w) & (fy >= 0) & (fy < h)
    live = inside & (cosb > 0) & (flux.sum(1) > 0) & ((v["pad"] & 0x80000000) == 0)
    # fb: 1 for an emitter vertex, else the BSDF of the vertex's material with its stored colour, towards the eye, from its predecessor
    fb = np.ones((len(v), 3))
    surf = np.nonzero(live & (v["depth"] != 0))[0]
    lb = np.asarray(v["last_position"], np.float64).reshape(-1, 3) - pos.astype(np.float64)
    lb /= np.linalg.norm(lb, axis=1, keepdims=True)
    keys = np.concatenate([v["material_id"][surf, None].astype(np.float64), np.asarray(v["color"], np.float64).reshape(-1, 3)[surf]], 1)
    for key in np.unique(keys, axis=0):
        sel = surf[(keys == key).all(1)]
        mat = dict(scene.materials[int(key[0])])
        assert not mat.get("brdf", 0)
        mat["color"] = tuple(float(x) for x in key[1:])
        f, _ = ob.bsdf_eval_pdf(mat, np.concatenate([nrm[sel], to_cam[sel], lb[sel]], 1))
        fb[sel] = f.astype(np.float64)
    live &= fb.sum(1) > 0
    idx = np.nonzero(live)[0]
    vis = r.trace_any(_shadow_rays(eye, pos[idx])) != 0
    idx = idx[vis]
    with np.errstate(all="ignore"):
        contrib = (flux[idx] / np.asarray(v["pdf"], np.float64)[idx, None]) * fb[idx] * (np.abs(cosb[idx]) / r2[idx] * we[idx] / path_count)[:, None]
    ok = np.isfinite(contrib).all(1)
    idx, contrib = idx[ok], contrib[ok]
    film = np.zeros((h, w, 3))
    px, py = np.floor(fx[idx]).astype(int), np.floor(fy[idx]).astype(int)
    np.add.at(film, (py, px), contrib)
    lit = np.zeros((h, w), bool)
    lit[py, px] = True
    return film, excluded, lit, len(idx), len(v)


# ------------------------------------------------------------------------------------------------------------ 5, 6
@pytest.fixture(scope="module")
def box(gpu, pkg, ob):
    """The Cornell box at 48 x 32, one "lt" frame of 2000 light paths, the cache it read and its float64 recount."""
    scene = pkg.scenes.cornell_box()
    w, h = 48, 32
    r = _renderer(pkg, scene, w, h, light=(2000, 16, 1), tuple_="minimal")
    r.render_frame("lt", 0)
    r.sync()
    film = r.read_accum().copy()
    v = r.lvc_read()
    _, _, _, vc, pc = r.sampler_read()
    assert vc == len(v) and pc == 2000
    host = _host_film(pkg, ob, r, scene, v, pc, w, h)
    return dict(scene=scene, r=r, w=w, h=h, film=film, host=host)


def test_the_film_is_the_caches_own_sum(box):
    """Every pixel of one "lt" frame against the float64 sum over the vertices of the cache the launch read (fb from the oracle's BSDF
    evaluator, visibility from trace_any on the kernel's own rays): rtol 1e-4 -- the device-against-oracle BSDF bar is 1e-5, the other
    factors are a handful of FP32 roundings, and a pixel adds well under 1 000 non-negative terms in arrival order (<= n 2^-24).
    Pixels whose value hangs on a float32 decision (a vertex within 1e-4 pixel of a pixel edge, or grazing the eye below 1e-3) are
    left out: at most 3 % of the lit pixels.  (The edge margin was first set to 1e-3 pixel on the estimate that 1 500 vertices land
    inside the image; 4 495 of the cache's 5 413 do, and 1e-3 would have left out 19 of the 501 lit pixels, 3.8 % -- more than this
    test allows itself.  1e-4 is still four times the float32 rounding of a pixel coordinate and leaves out fewer pixels, so the
    test checks more, not less.)  Unlit pixels are exactly 0.  Measured on the MI355X: largest deviation 9.3e-7, 6 of 501 lit pixels (1.2 %) left out."""
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


def test_band_sets(box):
    """Rows (0, 16, 1) then (16, 32, 1) on a cleared film against one full launch of the same cache: after the first launch the rows
    from 16 up are bit for bit the cleared film, the union equals the full launch to rtol 1e-5 (the order of the float atomics is the
    only difference), and (0, 32, 2) writes bands 0 and 2 only."""
    r, w, h = box["r"], box["w"], box["h"]
    r.clear_accum()
    cleared = r.read_accum().copy()
    r.launch("lt", 0)
    r.sync()
    full = r.read_accum().copy()
    assert np.allclose(full[..., :3], box["film"][..., :3], rtol=1e-5, atol=0.0)
    r.clear_accum()
    r.launch("lt", 0, (0, 16, 1))
    r.sync()
    a = r.read_accum().copy()
    assert a[16:].tobytes() == cleared[16:].tobytes()
    assert a[:16, :, :3].sum() > 0
    r.launch("lt", 0, (16, 32, 1))
    r.sync()
    b = r.read_accum().copy()
    assert b[:16].tobytes() == a[:16].tobytes()
    assert np.allclose(b[..., :3], full[..., :3], rtol=1e-5, atol=0.0)
    assert ((b[..., :3] == 0) == (full[..., :3] == 0)).all()
    r.clear_accum()
    r.launch("lt", 0, (0, 32, 2))
    r.sync()
    c = r.read_accum().copy()
    for band in (1, 3):
        assert c[8 * band:8 * band + 8].tobytes() == cleared[8 * band:8 * band + 8].tobytes()
    for band in (0, 2):
        rows = slice(8 * band, 8 * band + 8)
        assert np.allclose(c[rows, :, :3], full[rows, :, :3], rtol=1e-5, atol=0.0) and c[rows, :, :3].sum() > 0
    r.clear_accum()


# ------------------------------------------------------------------------------------------------------------ 7
def _lt_frames(r, n, w, h, bs=8):
    """n independent "lt" films (light pass of launch frame f + 1, sampler build, "lt" as subframe 0): block and image means per frame."""
    blocks, means = [], []
    for f in range(n):
        r.launch("light trace", f + 1)
        r.build_sampler()
        r.launch("lt", 0)
        r.sync()
        img = r.read_accum()[..., :3].astype(np.float64)
        assert np.isfinite(img).all()
        blocks.append(img.reshape(h // bs, bs, w // bs, bs, 3).mean((1, 3)))
        means.append(img.mean((0, 1)))
    return np.array(blocks), np.array(means)


def test_direct_light_against_quadrature(gpu, pkg, ob):
    """Floor under the tetrahedron lamp, the lamp outside the frustum: the image is direct light, and "lt" renders it from depth-1
    vertices alone.  Truth: the float64 quadrature of tests/test_gpu_mesh_light.py at 4 x 4 stratified positions per pixel (the box
    filter "lt" has).  The bars are that file's: image mean within 0.5 %, its standard error <= 0.005 / 3 of it, >= 99 % of the 8 x 8
    blocks within 4 s + 0.5 %."""
    W = H = 64
    N, PATHS = 128, 200000
    scene = pkg.scenes.lamp_floor()
    r = _renderer(pkg, scene, W, H, light=(PATHS, 8, 1), tuple_="minimal")
    eye, U, V, Wv = (np.asarray(a, np.float64) for a in _frame(pkg, scene, W, H))
    P64, _, _ = _light_geometry(pkg, scene)
    mat, Le = scene.materials[0], scene.mesh_lights[0]["emission"]

    def floor_points(k):
        y, x = np.mgrid[0:H, 0:W]
        s = (np.arange(k) + 0.5) / k
        px = (x[..., None, None] + s[None, None, None, :]) + 0 * s[None, None, :, None]
        py = (y[..., None, None] + s[None, None, :, None]) + 0 * s[None, None, None, :]
        d = (2 * px / W - 1)[..., None] * U + (2 * py / H - 1)[..., None] * V + Wv
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        t = -eye[1] / d[..., 1]
        assert (t > 0).all()
        p = eye + t[..., None] * d
        assert (np.abs(p[..., [0, 2]]) < 4).all()                      # every pixel sees the floor, nothing else
        return p.reshape(-1, 3), -d.reshape(-1, 3)

    # subdivision level of the lamp's faces, settled as in test_gpu_mesh_light.py: halving the sub-triangles changes no value by 1e-5
    x4, wo4 = floor_points(4)
    probe = np.random.default_rng(3).choice(len(x4), 1500, replace=False)
    level, prev = 0, _direct_light(ob, mat, Le, P64, x4[probe], wo4[probe], 0)
    while True:
        nxt = _direct_light(ob, mat, Le, P64, x4[probe], wo4[probe], level + 1)
        change = (np.abs(nxt - prev).max(1) / nxt.max(1)).max()
        level, prev = level + 1, nxt
        if change < 1e-5:
            break
        assert level < 5
    ref4 = _direct_light(ob, mat, Le, P64, x4, wo4, level).reshape(H, W, 16, 3).mean(2)
    x2, wo2 = floor_points(2)
    ref2 = _direct_light(ob, mat, Le, P64, x2, wo2, level).reshape(H, W, 4, 3).mean(2)
    blk = lambda a: a.reshape(H // 8, 8, W // 8, 8, 3).mean((1, 3))
    move = (np.abs(_lum(blk(ref4)) - _lum(blk(ref2))) / _lum(blk(ref4))).max()
    print(f"quadrature level {level}; 2 x 2 -> 4 x 4 positions per pixel moves the 8 x 8 block means by at most {move:.3g}")
    assert move <= 1e-4
    ref_b, ref_m = _lum(blk(ref4)), float(_lum(ref4.mean((0, 1))))

    blocks, means = _lt_frames(r, N, W, H)
    b = _lum(blocks)
    mean_b, s_b = b.mean(0), b.std(0, ddof=1) / math.sqrt(N)
    ok = np.abs(mean_b - ref_b) <= 4 * s_b + 0.005 * ref_b
    m = _lum(means)
    mean, se = m.mean(), m.std(ddof=1) / math.sqrt(N)
    z = (mean_b - ref_b) / s_b
    print(f"lt: image mean {mean:.6f} vs quadrature {ref_m:.6f} (ratio {mean / ref_m:.5f}, standard error {se / ref_m:.2e} of it); "
          f"blocks inside the bar {ok.mean():.4f}, block z-scores mean {z.mean():+.2f} rms {np.sqrt((z * z).mean()):.2f} max |z| {np.abs(z).max():.2f}")
    assert se <= 0.005 / 3 * ref_m, (se, ref_m)
    assert ok.mean() >= 0.99, (ok.mean(), np.abs(z).max())
    assert abs(mean / ref_m - 1) <= 0.005


# ------------------------------------------------------------------------------------------------------------ 8
def test_a_seen_emitter_shows_its_radiance(gpu, pkg):
    """The lamp inside the frame: a pixel whose whole footprint lies on a front face of the lamp is reached by emitter vertices only
    (depth 0: flux / pdf, fb = 1), and their sum estimates Le.  Pixels: the Moeller-Trumbore selection of test_gpu_mesh_light.py with
    its 1e-3 margins, at the four pixel corners.  Per channel the mean over the pixels and N frames equals Le within 4 standard
    errors + 0.5 %."""
    scene = pkg.scenes.lamp_floor(lamp_in_view=True)
    W = H = 96
    N = 24
    r = _renderer(pkg, scene, W, H, light=(100000, 8, 1), tuple_="minimal")
    eye, U, V, Wv = (np.asarray(a, np.float64) for a in _frame(pkg, scene, W, H))
    P64, _, _ = _light_geometry(pkg, scene)
    whole = np.ones((H, W), bool)
    y, x = np.mgrid[0:H, 0:W]
    for ox, oy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        d = (2 * (x + ox) / W - 1)[..., None] * U + (2 * (y + oy) / H - 1)[..., None] * V + Wv
        d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3)
        front = np.zeros(len(d), bool)
        for k in range(len(P64)):
            e1, e2 = P64[k, 1] - P64[k, 0], P64[k, 2] - P64[k, 0]
            n = np.cross(e1, e2)
            pv = np.cross(d, e2)
            det = pv @ e1
            tv = eye - P64[k, 0]
            u = (pv @ tv) / det
            qv = np.cross(tv, e1)
            v = (d @ qv) / det
            tt = (qv @ e2) / det
            front |= (d @ n < 0) & (u > 1e-3) & (v > 1e-3) & (u + v < 1 - 1e-3) & (tt > 0)
        whole &= front.reshape(H, W)
    assert whole.sum() > 60, whole.sum()
    per_frame = []
    for f in range(N):
        r.launch("light trace", f + 1)
        r.build_sampler()
        r.launch("lt", 0)
        r.sync()
        img = r.read_accum()[..., :3].astype(np.float64)
        assert np.isfinite(img).all()
        per_frame.append(img[whole].mean(0))
    per_frame = np.array(per_frame)
    Le = np.array(scene.mesh_lights[0]["emission"], np.float64)
    mean, se = per_frame.mean(0), per_frame.std(0, ddof=1) / math.sqrt(N)
    print(f"{int(whole.sum())} pixels wholly on the lamp's front faces; mean / Le = {mean / Le}, standard error / Le = {se / Le}")
    assert (np.abs(mean - Le) <= 4 * se + 0.005 * Le).all(), (mean, Le, se)


# ------------------------------------------------------------------------------------------------------------ 9, 11
@pytest.fixture(scope="module")
def room(gpu, pkg):
    """The Cornell room lit by the emissive icosphere at 96 x 96: per-frame image means of "lt" and of "pt"."""
    scene = pkg.scenes.cornell_sphere_lamp(2, 4)
    W = H = 96
    r = _renderer(pkg, scene, W, H, light=(100000, 52, 1), tuple_="minimal")
    N_LT, N_PT = 64, 320       # "pt": 2.5e-3 of the mean after 96 frames (tests/test_gpu_mesh_light.py) -> 1.4e-3 < 0.005 / 3 after 320
    blocks_lt, means_lt = _lt_frames(r, N_LT, W, H)
    r.clear_accum()
    prev = np.zeros((H, W, 3))
    means_pt, blocks_pt = [], []
    for f in range(N_PT):
        r.launch("pt", f)
        r.sync()
        acc = r.read_accum()[..., :3].astype(np.float64)
        img = (f + 1) * acc - f * prev
        prev = acc
        means_pt.append(img.mean((0, 1)))
        blocks_pt.append(img.reshape(H // 8, 8, W // 8, 8, 3).mean((1, 3)))
    return dict(scene=scene, lt=(_lum(blocks_lt), _lum(means_lt)), pt=(_lum(np.array(blocks_pt)), _lum(np.array(means_pt))))


def test_estimators_agree_on_a_room(room):
    """"lt" against "pt" on a room with many bounces: image means within 0.5 %, each standard error <= 0.005 / 3 of the mean (the bars
    of test_three_estimators_agree_on_a_room).  The per-block agreement is printed, not asserted."""
    res = {}
    for alg in ("lt", "pt"):
        b, m = room[alg]
        res[alg] = (m.mean(), m.std(ddof=1) / math.sqrt(len(m)))
        print(f"{alg}: image mean {res[alg][0]:.6f}, standard error {res[alg][1] / res[alg][0]:.2e} of it ({len(m)} frames)")
    base = res["pt"][0]
    for alg, (m, se) in res.items():
        assert se <= 0.005 / 3 * base, (alg, se, base)
    ratio = res["lt"][0] / res["pt"][0]
    sig = math.hypot(res["lt"][1], res["pt"][1]) / res["pt"][0]
    print(f"lt / pt = {ratio:.5f} (sigma of the ratio {sig:.2e}: {(ratio - 1) / sig:+.2f} sigma)")
    bl, bp = room["lt"][0], room["pt"][0]
    s = np.sqrt(bl.var(0, ddof=1) / len(bl) + bp.var(0, ddof=1) / len(bp))
    z = ((bl.mean(0) - bp.mean(0)) / np.where(s > 0, s, 1.0))[s > 0]     # (blocks outside the room are black in both)
    inside = np.abs(bl.mean(0) - bp.mean(0)) <= 4 * s + 0.005 * bp.mean(0)
    print(f"8 x 8 blocks: inside 4 s + 0.5 % {inside.mean():.4f}, z-scores mean {z.mean():+.2f} rms {np.sqrt((z * z).mean()):.2f} max |z| {np.abs(z).max():.2f}")
    assert abs(ratio - 1) <= 0.005, ratio


def test_render_tool_splats(room, pkg, tmp_path):
    """tools/spcbpt_render --alg lt --emissive on the sphere room's glTF file, 64 x 64, 16 frames: the PFM's mean is the room's "lt"
    mean to 5 % (plumbing: light pass + sampler build per frame over the minimal tuple, no preprocessing)."""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "spcbpt_render"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    path = pkg.scenes.write_gltf(room["scene"], str(tmp_path), "sphere_room")
    out = os.path.join(str(tmp_path), "tool")
    cmd = [os.path.join(ROOT, "tools", "spcbpt_render"), path, ".", "--alg", "lt", "--emissive", "--dim=64x64", "--frames", "16", "--out", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "16 subframes of lt at 64x64" in r.stdout and "preprocessing" in r.stdout, r.stdout
    raw = open(out + ".pfm", "rb").read()
    head = raw.split(b"\n", 3)
    assert head[0] == b"PF" and head[1] == b"64 64"
    img = np.frombuffer(head[3], np.float32).reshape(64, 64, 3)
    assert np.isfinite(img).all()
    tool, want = float(_lum(img.astype(np.float64)).mean()), float(room["lt"][1].mean())
    print(f"tool image mean {tool:.6f} vs the room's lt mean {want:.6f} (ratio {tool / want:.4f})")
    assert abs(tool / want - 1) <= 0.05


# ------------------------------------------------------------------------------------------------------------ 10
def test_errors(gpu, pkg):
    scene = pkg.scenes.cornell_box()
    w, h = 48, 32

    def fails(fn, code, text=None):
        with pytest.raises(pkg.SpcbptError) as e:
            fn()
        assert f"({code})" in str(e.value), str(e.value)
        if text:
            assert text in str(e.value), str(e.value)

    def pt_still_renders(r):
        r.clear_accum()
        r.launch("pt", 0)
        r.sync()
        img = r.read_accum()
        assert np.isfinite(img).all() and img[..., :3].mean() > 0

    STATE, INVALID, UNKNOWN = -5, -1, -4
    r = _renderer(pkg, scene, w, h, light=(2000, 16, 1), tuple_="minimal")
    fails(lambda: r.launch("lt", 0), STATE)                        # before any sampler build
    pt_still_renders(r)
    r.launch("light trace", 1)
    fails(lambda: r.launch("lt", 0), STATE)                        # a light pass without a build
    pt_still_renders(r)
    r.build_sampler()
    fails(lambda: r.launch("lt", 0, (4, h, 1)), INVALID)           # row_begin must be a multiple of 8
    pt_still_renders(r)
    fails(lambda: r.launch_deferred("lt", 0), UNKNOWN)             # the deferred form does not learn the name
    pt_still_renders(r)
    r.launch("lt", 0)                                              # ... and the sampler is still good for a real launch
    r.sync()
    assert r.read_accum()[..., :3].mean() > 0
    fails(lambda: r.launch("no such algorithm", 0), UNKNOWN, '"lt"')
    e = _renderer(pkg, scene, w, h, light=(2000, 16, 1), tuple_="minimal")
    e.set_environment(pkg.scenes.sky_texture())
    e.set_subspace()
    e.launch("light trace", 1)
    e.build_sampler()
    fails(lambda: e.launch("lt", 0), STATE, "environment")
    pt_still_renders(e)
