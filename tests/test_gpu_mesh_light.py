"""Mesh lights on the GPU (spcbpt_create_lit: the triangles of an emissive material as one area light).  The oracle knows quads only
and is not extended, so truth comes from places that do not run the code under test: the oracle's QUAD path on the same geometry
(a quad handed in as a two-triangle mesh light is the quad), a float64 quadrature of the direct light written here, the host
table (tests/test_mesh_light_host.py pins it to numpy), and first principles (where a sample lies, what a seen emitter shows).

Statistical bars.  A block / image mean is compared with its reference under |mean - ref| <= 4 s + 0.005 ref (s = the standard error
estimated from the per-frame means: 4 sigma lets ~0.01 % of the blocks out by chance) for >= 99 % of the blocks, and image means under
0.5 % -- the bar tests/test_gpu_configs.py holds SPCBPT == PT to -- with enough frames that the mean's own standard error is below a
third of that (asserted).  Counts of origins per triangle: Pearson chi^2 below its 1 - 1e-6 quantile (fixed frame: deterministic)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests.test_gpu_units import OP, _camera_records, _compare_steps, build_world, relerr

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ helpers
def _renderer(pkg, scene, w, h, light=(20000, 16, 1), tuple_=None):
    cam = scene.camera
    r = pkg.Renderer(scene, 0)
    U, V, W = pkg.camera_frame(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
    r.set_camera(np.array(cam["eye"], np.float32), U, V, W)
    r.resize(w, h)
    r.set_light_trace(*light)
    if tuple_ == "minimal":
        r.set_subspace()
    elif tuple_ == "trained":
        r.set_pretrace(20000, 10)
        r.preprocess(target_paths=100000, target_q_paths=100000, train=True)
    elif tuple_ is not None:
        r.set_subspace(*tuple_)
    return r


def _chi2_sf(x, df):
    """P(chi^2_df > x) in closed form (integer df)."""
    h = 0.5 * x
    if df % 2 == 0:
        term, s = 1.0, 1.0
        for k in range(1, df // 2):
            term *= h / k
            s += term
        return math.exp(-h) * s
    s, term = 0.0, math.sqrt(h) / math.gamma(1.5)
    for k in range(1, (df - 1) // 2 + 1):
        s += term
        term *= h / (k + 0.5)
    return math.erfc(math.sqrt(h)) + math.exp(-h) * s


def test_chi2_tail_helper():
    assert abs(_chi2_sf(30.6648, 3) - 1e-6) < 2e-8 and abs(_chi2_sf(3.8415, 1) - 0.05) < 1e-4 and abs(_chi2_sf(18.307, 10) - 0.05) < 1e-4


def _light_geometry(pkg, scene, k=0):
    """Corners (n, 3, 3) float64 of the triangles of mesh light k in the order of the host table, with the table."""
    ml = scene.mesh_lights[k]
    F = np.asarray(scene.indices)[np.asarray(scene.tri_material) == ml["material"]]
    t = pkg.api.mesh_light_table(scene.vertices, F, ml.get("n_patches", 4))
    P = np.asarray(scene.vertices, np.float32)[F[t["tri"]]]
    return P.astype(np.float64), P, t


def _locate(P, x):
    """For points x (m, 3): the triangle of P (n, 3, 3) each lies on -> (index, barycentrics (m, 3), plane distance)."""
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    n = np.cross(e1, e2)
    nn = n / np.linalg.norm(n, axis=1, keepdims=True)
    best = np.full(len(x), -1)
    best_cost = np.full(len(x), np.inf)
    bary = np.zeros((len(x), 3))
    dist = np.zeros(len(x))
    for k in range(len(P)):
        d = x - P[k, 0]
        pd = d @ nn[k]
        q = d - pd[:, None] * nn[k]
        den = n[k] @ n[k]
        b1 = np.cross(q, e2[k]) @ n[k] / den
        b2 = np.cross(e1[k], q) @ n[k] / den
        b = np.stack([1 - b1 - b2, b1, b2], 1)
        cost = np.abs(pd) + np.maximum(0.0, -b.min(1)) * np.sqrt(den)
        better = cost < best_cost
        best[better], best_cost[better], bary[better], dist[better] = k, cost[better], b[better], np.abs(pd[better])
    return best, bary, dist


def _pearson(counts, expected):
    """chi^2 and degrees of freedom after merging cells that expect fewer than five (in table order)."""
    order = np.argsort(expected)
    c, e = counts[order].astype(np.float64), expected[order].astype(np.float64)
    cells_c, cells_e, ac, ae = [], [], 0.0, 0.0
    for a, b in zip(c, e):
        ac += a; ae += b
        if ae >= 5.0:
            cells_c.append(ac); cells_e.append(ae); ac = ae = 0.0
    if ae > 0:
        cells_c[-1] += ac; cells_e[-1] += ae
    cc, ee = np.array(cells_c), np.array(cells_e)
    return float(((cc - ee) ** 2 / ee).sum()), len(cc) - 1


def _frames(r, alg, n, w, h, bs=8):
    """n frames of `alg`; returns (final accum rgb, per-frame block means (n, h/bs, w/bs, 3), per-frame image means (n, 3))."""
    r.clear_accum()
    prev = np.zeros((h, w, 3))
    blocks, means = [], []
    for f in range(n):
        r.render_frame(alg, f)
        r.sync()
        acc = r.read_accum()[..., :3].astype(np.float64)
        img = (f + 1) * acc - f * prev          # the film keeps the running mean: frame f's own samples
        prev = acc
        blocks.append(img.reshape(h // bs, bs, w // bs, bs, 3).mean((1, 3)))
        means.append(img.mean((0, 1)))
    return prev, np.array(blocks), np.array(means)


def _lum(rgb):
    return np.asarray(rgb)[..., :3].sum(-1)


# ------------------------------------------------------------------------------------------------------------ 3, 8
@pytest.fixture(scope="module")
def quad_and_mesh(gpu, pkg, ob):
    """Scene Q: the Cornell box with its quad light (one patch).  Scene M: the same box, the quad's two triangles as scene geometry
    under a material named as a mesh light.  The same trained tuple and the same light-vertex cache in both products and the oracle."""
    q = pkg.scenes.cornell_box(div_level=1)
    world = build_world(pkg, ob, q)
    m = pkg.scenes.quad_lights_as_mesh(q, n_patches=1)
    rm = _renderer(pkg, m, world["W"], world["H"], light=(8000, 64, 1), tuple_=world["tup"])
    cam = q.camera
    rm.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], world["W"] / world["H"])
    rm.lvc_import(world["lvc"]); rm.build_sampler()
    world["rm"], world["mesh_scene"] = rm, m
    return world


def test_a_quad_given_as_a_mesh_is_the_quad(quad_and_mesh, pkg, ob):
    """The SPCBPT_UNIT_EYE_STEP chain of test_eye_step_connection_and_emitter_hit_chain, four levels, the product in context M
    against the ORACLE on scene Q under that test's own bars (kinds, surface vertices, emitter radiance 1e-4 for 99.8 %, 1e-3 hard;
    back hits exactly 0), more than 20 emitter hits at depth >= 2 (their value carries the rmis::light_hit weight: a wrong pdf,
    normal or label on the mesh branch shows there); and the product in Q against the product in M on every record to 1e-5 (the
    area: two triangle areas summed in double against |u x v| in float)."""
    w = quad_and_mesh
    rq, rm, o = w["r"], w["rm"], w["o"]
    iq, im = rq.light_info(), rm.light_info()
    assert [x["type"] for x in iq] == [0] and [x["type"] for x in im] == [2]
    assert im[0]["n_triangles"] == 2 and im[0]["n_patches"] == 1 and im[0]["first_subspace"] == iq[0]["first_subspace"] == 999
    assert abs(im[0]["area"] - iq[0]["area"]) <= 1e-6 * iq[0]["area"]
    rng = np.random.default_rng(8)
    rec = _camera_records(pkg, ob, w, 16384, rng)
    deep_emit = 0
    for level in range(1, 5):
        want = o.eye_step(rec)
        words = rec.view(np.uint32).reshape(len(rec), -1)
        got_m = rm.unit(OP["EYE_STEP"], words, 40)
        got_q = rq.unit(OP["EYE_STEP"], words, 40)
        _, n_emit = _compare_steps(ob, got_m, want, level)
        deep_emit += n_emit if level > 1 else 0
        gm, gq = (g.view(ob.EYE_STEP_OUT_DTYPE).reshape(-1) for g in (got_m, got_q))
        assert np.array_equal(gm["kind"], gq["kind"]), level
        hit = gq["kind"] == 2
        e = relerr(gm["emit"][hit], gq["emit"][hit])
        print(f"level {level}: {int(hit.sum())} emitter hits, product(M) vs product(Q) max rel {e.max() if len(e) else 0:.3g}")
        assert len(e) == 0 or e.max() <= 1e-5, (level, e.max())
        assert np.array_equal(gm["emit"][~hit], gq["emit"][~hit])
        # the light's record at the hit: same label, same normal, same pdf up to the area's rounding
        assert np.array_equal(gm["mid"]["subspace_id"][hit], gq["mid"]["subspace_id"][hit])
        assert relerr(gm["mid"]["pdf"][hit], gq["mid"]["pdf"][hit]).max(initial=0) <= 1e-6
        assert np.abs(gm["mid"]["normal"][hit] - gq["mid"]["normal"][hit]).max(initial=0) <= 1e-6
        surf = gq["kind"] == 1
        assert np.array_equal(gm["mid"][surf], gq["mid"][surf])
        go = (want["kind"] == 1) & (want["done"] == 0)
        nxt = np.zeros(int(go.sum()), ob.EYE_STEP_IN_DTYPE)
        nxt["last"] = want["mid"][go]; nxt["next_flux"] = want["next_flux"][go]; nxt["next_single_pdf"] = want["next_single_pdf"][go]
        nxt["seed"] = want["seed"][go]; nxt["dir"] = want["dir"][go]
        rec = nxt
        assert len(rec) > 300 or level == 4, level
    assert deep_emit > 20


def test_origin_vertices_connect_like_a_quads(quad_and_mesh, pkg):
    """Same frame number in Q and M: the depth-0 vertices of the two caches agree in everything but the position (another
    sampler), and 200 frames of SPCBPT_eye give the same image mean."""
    w = quad_and_mesh
    rq, rm = w["r"], w["rm"]
    caches = []
    for r in (rq, rm):
        r.launch("light trace", 21)
        v = r.lvc_read()
        caches.append(v[v["depth"] == 0])
    a, b = caches
    assert len(a) == len(b) == 8000 and np.array_equal(a["path_id"], b["path_id"])
    for k in ("pdf", "single_pdf"):
        assert relerr(b[k], a[k]).max() <= 1e-6, k
    assert np.abs(a["normal"] - b["normal"]).max() <= 1e-6
    for k in ("flux", "rmis_pointer", "subspace_id", "material_id", "depth", "last_zone_id", "pad"):
        assert np.array_equal(a[k], b[k]), k
    # both samplers cover the quad: the mesh's points lie on it
    lo, hi = a["position"].min(0), a["position"].max(0)
    assert (b["position"] >= lo - 1e-3).all() and (b["position"] <= hi + 1e-3).all() and np.abs(b["position"].mean(0) - a["position"].mean(0)).max() < 0.01
    # 200 frames; the image mean's noise is that of the light pass every pixel shares, so the frames get more light paths (and
    # pixels) than the function-level checks above need
    W, H, N = 256, 144, 200
    stats = []
    for r in (rq, rm):
        r.resize(W, H)
        r.set_light_trace(100000, 32, 1)
        _, _, means = _frames(r, "SPCBPT_eye", N, W, H)
        m = _lum(means)
        stats.append((m.mean(), m.std(ddof=1) / math.sqrt(N)))
    (mq, sq), (mm, sm) = stats
    print(f"SPCBPT_eye image mean: quad {mq:.6f} +- {sq:.2g}, mesh {mm:.6f} +- {sm:.2g}, ratio {mm / mq:.5f}")
    assert max(sq, sm) <= 0.005 / 3 * mq, (sq, sm, mq)
    assert abs(mm / mq - 1) <= 0.005


# ------------------------------------------------------------------------------------------------------------ 4, 5
@pytest.fixture(scope="module")
def lamp(gpu, pkg):
    scene = pkg.scenes.lamp_floor()
    r = _renderer(pkg, scene, 64, 64, light=(40000, 16, 1), tuple_="minimal")
    return dict(scene=scene, r=r)


def _check_origins(pkg, r, scene, frame, n_paths, light_index=0, n_lights=1):
    r.launch("light trace", frame)
    v = r.lvc_read()
    o = v[v["depth"] == 0]
    assert len(o) == n_paths and np.array_equal(o["path_id"], np.arange(n_paths, dtype=np.uint32))     # one origin per path, as for quads
    o = o[o["material_id"] == light_index]
    P64, P32, t = _light_geometry(pkg, scene)
    extent = float(np.linalg.norm(scene.vertices.max(0) - scene.vertices.min(0)))
    tri, bary, dist = _locate(P64, o["position"].astype(np.float64))
    assert bary.min() >= -1e-5 and bary.max() <= 1 + 1e-5, (bary.min(), bary.max())
    assert dist.max() <= 1e-5 * extent, dist.max()
    n = np.cross(P64[:, 1] - P64[:, 0], P64[:, 2] - P64[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    # (a point within rounding of an edge may be attributed to the neighbour: only points clearly inside are held to the triangle)
    inside = bary.min(1) > 1e-4
    assert inside.mean() > 0.99
    assert np.abs(o["normal"][inside] - n[tri[inside]]).max() <= 1e-6
    info = r.light_info()[light_index]
    assert info["type"] == 2 and info["n_triangles"] == len(P64) and info["n_patches"] == t["n_patches"]
    assert abs(info["area"] - t["area"]) <= 1e-6 * t["area"]
    pdf = (1.0 / t["area"]) / n_lights
    assert relerr(o["pdf"], np.full(len(o), pdf)).max() <= 1e-6 and np.array_equal(o["pdf"], o["single_pdf"])
    assert np.array_equal(o["subspace_id"][inside], (info["first_subspace"] - t["patch"][tri[inside]]).astype(np.int16))
    assert set(o["subspace_id"]) <= set(range(info["first_subspace"] - t["n_patches"] + 1, info["first_subspace"] + 1))
    assert np.array_equal(o["flux"], np.tile(np.array(scene.mesh_lights[0]["emission"], np.float32), (len(o), 1)))
    assert (o["rmis_pointer"] == 1).all() and (o["pad"] == 0).all()
    counts = np.bincount(tri, minlength=len(P64))
    share = np.diff(np.concatenate([[0.0], t["cmf"].astype(np.float64)]))
    chi2, df = _pearson(counts, share * len(o))
    p = _chi2_sf(chi2, df)
    print(f"{scene.name}: {len(o)} origins on {len(P64)} triangles: chi^2 = {chi2:.1f} with {df} degrees of freedom (tail probability {p:.3g})")
    assert p > 1e-6, (chi2, df)
    return o, tri, inside


def test_origin_vertices_lie_on_the_light(lamp, pkg):
    o, tri, inside = _check_origins(pkg, lamp["r"], lamp["scene"], 7, 40000)
    lamp["origins"] = (o, tri, inside)
    # ... and on a light of many triangles (the guide-table search over a 320-entry CMF)
    sph = pkg.scenes.cornell_sphere_lamp()
    r = _renderer(pkg, sph, 64, 64, light=(40000, 16, 1), tuple_="minimal")
    _check_origins(pkg, r, sph, 7, 40000)


def test_one_quad_and_one_mesh_light_share_the_origins(gpu, pkg):
    scene = pkg.scenes.lamp_floor()
    scene.lights = [dict(position=(-2.0, 3.0, -2.0), u=(1.0, 0, 0), v=(0, 0, 1.0), emission=(5, 5, 5), div_level=2)]
    r = _renderer(pkg, scene, 64, 64, light=(40000, 16, 1), tuple_="minimal")
    info = r.light_info()
    assert [x["type"] for x in info] == [0, 2] and info[0]["first_subspace"] == 999 and info[1]["first_subspace"] == 995
    r.launch("light trace", 7)
    v = r.lvc_read()
    o = v[v["depth"] == 0]
    n, k = len(o), int((o["material_id"] == 1).sum())
    print(f"{k} of {n} origins on the mesh light ({(k - 0.5 * n) / math.sqrt(0.25 * n):+.2f} sigma)")
    assert n == 40000 and abs(k - 0.5 * n) <= 5 * math.sqrt(0.25 * n)
    assert set(o["subspace_id"][o["material_id"] == 0]) <= {999, 998, 997, 996}
    assert set(o["subspace_id"][o["material_id"] == 1]) <= {995, 994, 993, 992}
    _check_origins(pkg, r, scene, 9, 40000, light_index=1, n_lights=2)


def test_hit_and_sample_agree_on_label_and_pdf(lamp, pkg, ob):
    if "origins" not in lamp:
        lamp["origins"] = _check_origins(pkg, lamp["r"], lamp["scene"], 7, 40000)
    o, tri, inside = lamp["origins"]
    scene, r = lamp["scene"], lamp["r"]
    pick = np.nonzero(inside)[0][:4096]
    assert len(pick) >= 1000
    s = o[pick]
    extent = np.float32(np.linalg.norm(scene.vertices.max(0) - scene.vertices.min(0)))
    rec = np.zeros(len(pick), ob.EYE_STEP_IN_DTYPE)
    start = (s["position"] + s["normal"] * (np.float32(1e-2) * extent)).astype(np.float32)
    rec["last"]["position"] = start; rec["last"]["normal"] = -s["normal"]; rec["last"]["flux"] = 1.0
    rec["last"]["last_position"] = start; rec["last"]["pdf"] = 1.0; rec["last"]["single_pdf"] = 1.0
    rec["next_single_pdf"] = 1.0; rec["seed"] = 1; rec["dir"] = -s["normal"]
    out = r.unit(OP["EYE_STEP"], rec.view(np.uint32).reshape(len(rec), -1), 40).view(ob.EYE_STEP_OUT_DTYPE).reshape(-1)
    assert (out["kind"] == 2).all()
    assert np.abs(out["t_hit"] - 1e-2 * extent).max() <= 1e-4 * extent
    assert np.array_equal(out["mid"]["subspace_id"], s["subspace_id"].astype(np.int32))
    assert np.array_equal(out["mid"]["pdf"].view(np.uint32), s["pdf"].view(np.uint32))          # bit-equal
    assert np.abs(out["mid"]["normal"] - s["normal"]).max() <= 1e-6
    # depth 0: the radiance itself, up to the rounding of flux / pdf (the geometry term is multiplied in and divided out in FP32, as for a quad)
    assert relerr(out["emit"], np.tile(np.array(scene.mesh_lights[0]["emission"], np.float32), (len(s), 1))).max() <= 1e-6
    # from inside the closed lamp every face shows its back: single-sided, the ray passes (emits nothing)
    c = scene.vertices[np.unique(scene.indices[scene.tri_material == 1])].mean(0).astype(np.float32)
    rec["last"]["position"] = c; rec["last"]["last_position"] = c
    d = (s["position"] - c); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rec["last"]["normal"] = d; rec["dir"] = d
    out = r.unit(OP["EYE_STEP"], rec.view(np.uint32).reshape(len(rec), -1), 40).view(ob.EYE_STEP_OUT_DTYPE).reshape(-1)
    assert (out["kind"] != 2).all() and (out["emit"] == 0).all()


# ------------------------------------------------------------------------------------------------------------ 6
def _tea4(v0, v1):
    v0, v1 = np.asarray(v0, np.uint32).copy(), np.asarray(v1, np.uint32).copy()
    s0 = np.uint32(0)
    with np.errstate(over="ignore"):
        for _ in range(4):
            s0 = np.uint32(s0 + np.uint32(0x9e3779b9))
            v0 += ((v1 << np.uint32(4)) + np.uint32(0xa341316c)) ^ (v1 + s0) ^ ((v1 >> np.uint32(5)) + np.uint32(0xc8013ea4))
            v1 += ((v0 << np.uint32(4)) + np.uint32(0xad90777d)) ^ (v0 + s0) ^ ((v0 >> np.uint32(5)) + np.uint32(0x7e95761e))
    return v0


def _rnd(seed):
    with np.errstate(over="ignore"):
        seed = np.uint32(1664525) * seed + np.uint32(1013904223)
    return seed, (seed & np.uint32(0x00FFFFFF)).astype(np.float32) / np.float32(0x01000000)


def _jitter(w, h, subframe):
    """The pixel positions the camera draws in `subframe` (camera_ray: tea<4>(pixel, subframe), two numbers; the centre in frame 0)."""
    y, x = np.mgrid[0:h, 0:w]
    if subframe == 0:
        return x + 0.5, y + 0.5
    seed = _tea4((y * w + x).astype(np.uint32), np.full((h, w), subframe, np.uint32))
    seed, jx = _rnd(seed)
    seed, jy = _rnd(seed)
    return x + jx.astype(np.float64), y + jy.astype(np.float64)


_DUNAVANT7 = (np.array([[1 / 3, 1 / 3, 1 / 3]] + [p for a, b in ((0.059715871789770, 0.470142064105115), (0.797426985353087, 0.101286507323456))
                                                  for p in ([a, b, b], [b, a, b], [b, b, a])]),
              np.array([0.225] + [0.132394152788506] * 3 + [0.125939180544827] * 3))


def _quadrature_nodes(P, level):
    """Nodes and weights (area measure) of the degree-5 seven-point rule on the 4^level sub-triangles of each triangle of P (n, 3, 3)."""
    tris = P
    for _ in range(level):
        a, b, c = tris[:, 0], tris[:, 1], tris[:, 2]
        ab, bc, ca = 0.5 * (a + b), 0.5 * (b + c), 0.5 * (c + a)
        tris = np.concatenate([np.stack(t, 1) for t in ((a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca))])
    bary, wt = _DUNAVANT7
    nodes = np.einsum("qk,nkd->nqd", bary, tris)
    area = 0.5 * np.linalg.norm(np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]), axis=1)
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    owner = np.tile(np.arange(len(P)), 4 ** level)
    return nodes.reshape(-1, 3), (area[:, None] * wt[None, :]).reshape(-1), np.repeat(nrm[owner], len(wt), axis=0)


def _direct_light(ob, mat, Le, P, x, wo, level, chunk=2048):
    """Float64 direct radiance (m, 3) leaving floor points x (normal +y) towards wo, from the front sides of the lamp's faces P:
    sum over the quadrature nodes of Le f(wo, wi) cos cos' / r^2 dA, f from the oracle's BSDF evaluator (tests/test_gpu_units.py
    pins it).  A convex closed lamp: a face whose front a floor point sees is unoccluded."""
    nodes, wts, nrm = _quadrature_nodes(P, level)
    out = np.zeros((len(x), 3))
    N = np.array([0.0, 1.0, 0.0])
    for s in range(0, len(x), chunk):
        xs, ws = x[s:s + chunk], wo[s:s + chunk]
        d = nodes[None, :, :] - xs[:, None, :]
        r2 = (d * d).sum(-1)
        wi = d / np.sqrt(r2)[..., None]
        cos_s = wi[..., 1]
        cos_l = -(wi * nrm[None, :, :]).sum(-1)
        g = np.where((cos_s > 0) & (cos_l > 0), cos_s * cos_l / r2, 0.0) * wts[None, :]
        nvl = np.concatenate([np.broadcast_to(N, wi.shape), np.broadcast_to(ws[:, None, :], wi.shape), wi], -1).reshape(-1, 9)
        f, _ = ob.bsdf_eval_pdf(mat, nvl)
        out[s:s + chunk] = (f.astype(np.float64).reshape(wi.shape) * g[..., None]).sum(1) * np.asarray(Le, np.float64)[None, :]
    return out


@pytest.fixture(scope="module")
def lamp_truth(gpu, pkg, ob):
    """Scene, renderer with a trained tuple, and the float64 reference of every block of every frame's jittered pixel positions."""
    W = H = 64
    N = 256      # "pt" is the noisiest of the three here: 2.6e-3 of the mean after 64 frames, so 256 bring it to 1.3e-3 < 0.005 / 3
    scene = pkg.scenes.lamp_floor()
    r = _renderer(pkg, scene, W, H, light=(20000, 16, 1), tuple_="trained")
    cam = scene.camera
    eye = np.array(cam["eye"], np.float64)
    U, V, Wv = (np.asarray(a, np.float64) for a in pkg.camera_frame(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H))
    P64, _, _ = _light_geometry(pkg, scene)
    xs, wos = [], []
    for f in range(N):
        px, py = _jitter(W, H, f)
        d = (2 * px / W - 1)[..., None] * U + (2 * py / H - 1)[..., None] * V + Wv
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        t = -eye[1] / d[..., 1]
        assert (t > 0).all()
        x = eye + t[..., None] * d
        assert (np.abs(x[..., [0, 2]]) < 4).all()                         # every pixel sees the floor, nothing else
        xs.append(x.reshape(-1, 3)); wos.append(-d.reshape(-1, 3))
    x, wo = np.concatenate(xs), np.concatenate(wos)
    mat, Le = scene.materials[0], scene.mesh_lights[0]["emission"]
    # fixed order: the subdivision level at which halving the sub-triangles changes no value by 1e-5 (settled on a sample of the points)
    probe = np.random.default_rng(3).choice(len(x), 1500, replace=False)
    level, prev = 0, _direct_light(ob, mat, Le, P64, x[probe], wo[probe], 0)
    while True:
        nxt = _direct_light(ob, mat, Le, P64, x[probe], wo[probe], level + 1)
        change = (np.abs(nxt - prev).max(1) / nxt.max(1)).max()
        print(f"quadrature: level {level} -> {level + 1} changes the direct light by at most {change:.3g}")
        level, prev = level + 1, nxt
        if change < 1e-5:
            break
        assert level < 5
    ref = _direct_light(ob, mat, Le, P64, x, wo, level).reshape(N, H, W, 3)
    return dict(scene=scene, r=r, W=W, H=H, N=N, ref_blocks=ref.reshape(N, H // 8, 8, W // 8, 8, 3).mean((0, 2, 4)), ref_mean=ref.mean((0, 1, 2)))


@pytest.mark.parametrize("alg", ["pt", "SPCBPT_eye", "SPCBPT_no_rmis"])
def test_direct_light_against_quadrature(lamp_truth, alg):
    """Floor under the tetrahedron lamp, camera on the floor only: the image is direct light.  Per 8 x 8 block: |mean - ref| <= 4 s +
    0.005 ref for >= 99 % of the blocks; image mean within 0.5 % of the reference's, its standard error below a third of that."""
    t = lamp_truth
    N, W, H = t["N"], t["W"], t["H"]
    acc, blocks, means = _frames(t["r"], alg, N, W, H)
    assert np.isfinite(acc).all()
    ref_b, ref_m = _lum(t["ref_blocks"]), float(_lum(t["ref_mean"]))
    b = _lum(blocks)
    mean_b, s_b = b.mean(0), b.std(0, ddof=1) / math.sqrt(N)
    ok = np.abs(mean_b - ref_b) <= 4 * s_b + 0.005 * ref_b
    m = _lum(means)
    mean, se = m.mean(), m.std(ddof=1) / math.sqrt(N)
    z = (mean_b - ref_b) / s_b
    print(f"{alg}: image mean {mean:.6f} vs quadrature {ref_m:.6f} (ratio {mean / ref_m:.5f}, standard error {se / ref_m:.2e} of it); "
          f"blocks inside the bar {ok.mean():.4f}, block z-scores mean {z.mean():+.2f} rms {np.sqrt((z * z).mean()):.2f} max |z| {np.abs(z).max():.2f}")
    assert se <= 0.005 / 3 * ref_m, (se, ref_m)
    assert ok.mean() >= 0.99, (ok.mean(), np.abs(z).max())
    assert abs(mean / ref_m - 1) <= 0.005


@pytest.mark.parametrize("alg", ["pt", "SPCBPT_eye", "SPCBPT_no_rmis"])
def test_a_seen_lamp_shows_its_radiance(gpu, pkg, alg):
    """The lamp inside the frame, frame 0 (rays through the pixel centres): a pixel whose ray hits a lamp face from the front shows Le
    (a depth-0 emitter hit carries no weight).  "pt" adds the emission itself: exactly Le.  The two SPCBPT forms evaluate flux / pdf,
    which carries the geometry term in the numerator and in the denominator (eye_emitter_hit, eval_path; a quad light rounds the
    same way): Le to 1e-6 relative, i.e. a few FP32 roundings (measured on the MI355X: 1.4e-7 at most)."""
    scene = pkg.scenes.lamp_floor(lamp_in_view=True)
    W = H = 96
    r = _renderer(pkg, scene, W, H, light=(20000, 16, 1), tuple_="minimal")
    r.render_frame(alg, 0)
    r.sync()
    img = r.read_accum()[..., :3]
    cam = scene.camera
    eye = np.array(cam["eye"], np.float64)
    U, V, Wv = (np.asarray(a, np.float64) for a in pkg.camera_frame(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H))
    px, py = _jitter(W, H, 0)
    d = (2 * px / W - 1)[..., None] * U + (2 * py / H - 1)[..., None] * V + Wv
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3)
    P64, _, _ = _light_geometry(pkg, scene)
    front = np.zeros(len(d), bool)
    for k in range(len(P64)):                                         # Moller-Trumbore, clearly inside a face seen from its front
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
    Le = np.array(scene.mesh_lights[0]["emission"], np.float32)
    seen = img.reshape(-1, 3)[front]
    dev = np.abs(seen.astype(np.float64) - Le).max() / Le.max() if len(seen) else 0.0
    print(f"{alg}: {int(front.sum())} pixels on the lamp's front faces, max deviation from Le {dev:.3g}")
    assert front.sum() > 100
    if alg == "pt":
        assert np.array_equal(seen, np.tile(Le, (len(seen), 1))), dev
    assert dev <= 1e-6, dev
    assert np.isfinite(img).all()


# ------------------------------------------------------------------------------------------------------------ 7, 9
@pytest.fixture(scope="module")
def sphere_room(gpu, pkg, tmp_path_factory):
    """The Cornell room lit only by an emissive icosphere (320 triangles, 4 patches), loaded through the glTF route."""
    d = tmp_path_factory.mktemp("sphere_room")
    src = pkg.scenes.cornell_sphere_lamp(subdivisions=2, n_patches=4)
    path = pkg.scenes.write_gltf(src, str(d), "sphere_room")
    scene, warn = pkg.load_gltf(path, emissive=True)
    assert scene.lights == [] and len(scene.mesh_lights) == 1 and scene.mesh_lights[0]["n_patches"] == 4, warn
    assert np.array_equal(np.array(scene.mesh_lights[0]["emission"], np.float32), np.array(src.mesh_lights[0]["emission"], np.float32))
    scene.camera = dict(src.camera)
    return dict(scene=scene, dir=d)


def test_three_estimators_agree_on_a_room(sphere_room, pkg):
    scene = sphere_room["scene"]
    W = H = 96
    N = 320      # "pt": 2.5e-3 of the mean after 96 frames -> 1.4e-3 < 0.005 / 3
    r = _renderer(pkg, scene, W, H, light=(20000, 32, 1), tuple_="trained")
    info = r.light_info()
    assert len(info) == 1 and info[0]["type"] == 2 and info[0]["n_triangles"] == 320 and info[0]["n_patches"] == 4
    sphere_room["tuple"] = r.get_subspace()
    res = {}
    for alg in ("pt", "SPCBPT_eye", "SPCBPT_no_rmis"):
        acc, _, means = _frames(r, alg, N, W, H)
        assert np.isfinite(acc).all(), alg
        m = _lum(means)
        res[alg] = (m.mean(), m.std(ddof=1) / math.sqrt(N))
        print(f"{alg}: image mean {res[alg][0]:.6f}, standard error {res[alg][1] / res[alg][0]:.2e} of it")
    base = res["pt"][0]
    for alg, (m, se) in res.items():
        assert se <= 0.005 / 3 * base, (alg, se, base)
    for a, b in (("SPCBPT_eye", "pt"), ("SPCBPT_no_rmis", "pt"), ("SPCBPT_eye", "SPCBPT_no_rmis")):
        ratio = res[a][0] / res[b][0]
        sig = math.hypot(res[a][1], res[b][1]) / res[b][0]
        print(f"{a} / {b} = {ratio:.5f} (sigma of the ratio {sig:.2e}: {(ratio - 1) / sig:+.2f} sigma)")
        assert abs(ratio - 1) <= 0.005, (a, b, ratio)
    # kernel times against the same room lit by a quad of equal area and emission (figures for DESIGN.md; no bar)
    area = info[0]["area"]
    side = math.sqrt(area)
    quad = pkg.scenes.cornell_sphere_lamp()
    quad.indices, quad.tri_material = quad.indices[quad.tri_material != 3], quad.tri_material[quad.tri_material != 3]
    quad.mesh_lights = []
    quad.lights = [dict(position=(0.05 - side / 2, 1.998, 0.1 - side / 2), u=(side, 0, 0), v=(0, 0, side), emission=scene.mesh_lights[0]["emission"], div_level=2)]
    rq = _renderer(pkg, quad, W, H, light=(20000, 32, 1), tuple_="minimal")
    r.set_subspace()
    for name, x in (("mesh light", r), ("quad light", rq)):
        x.enable_kernel_timing(True)
        x.reset_kernel_time()
        for f in range(20):
            x.launch("light trace", 100 + f)
            x.launch("pt", f)
        x.sync()
        print(f"kernel times, {name}: light trace {x.kernel_time('light_trace')[0]:.4f} ms, pt {x.kernel_time('pt')[0]:.4f} ms")
        x.enable_kernel_timing(False)


def test_every_launch_form_renders_the_same_film(sphere_room, pkg, tmp_path):
    scene = sphere_room["scene"]
    W = H = 96
    FR = 4

    def make(env=None):
        for k, v in (env or {}).items():
            os.environ[k] = v
        try:
            return _renderer(pkg, scene, W, H, light=(3000, 32, 1), tuple_="minimal")
        finally:
            for k in (env or {}):
                del os.environ[k]
    a = make()
    for f in range(FR):
        a.launch("light trace", f + 1); a.build_sampler(); a.launch("SPCBPT_eye", f)
    a.sync()
    want = a.read_accum().copy()
    assert np.isfinite(want).all() and want[..., :3].mean() > 0
    tup = a.get_subspace()
    # batched eye launch
    b = make({"SPCBPT_EYE_BATCH": "4"})
    b.set_subspace(*tup)
    for f in range(FR):
        b.launch("light trace", f + 1); b.build_sampler()
    b.launch_eye_batch(list(range(FR)))
    b.sync()
    assert np.array_equal(b.read_accum(), want)
    # deferred launch + merge
    c = make()
    c.set_subspace(*tup)
    for f in range(FR):
        c.launch("light trace", f + 1); c.build_sampler(); c.launch_deferred("SPCBPT_eye", f); c.merge_deferred(True)
    c.sync()
    assert np.array_equal(c.read_accum(), want)
    # light passes one frame ahead
    c.clear_accum()
    c.set_light_ahead(True)
    c.launch("light trace", 1)
    for f in range(FR):
        c.launch("light trace", f + 2); c.build_sampler(); c.launch("SPCBPT_eye", f)
    c.sync()
    assert np.array_equal(c.read_accum(), want)
    c.set_light_ahead(False)
    # "pt": plain and deferred
    a.clear_accum(); c.clear_accum()
    for f in range(FR):
        a.launch("pt", f)
        c.launch_deferred("pt", f); c.merge_deferred(True)
    a.sync(); c.sync()
    assert np.array_equal(a.read_accum(), c.read_accum())
    # checkpoint round trip of a trained tuple
    a.set_pretrace(8000, 10)
    a.preprocess(target_paths=30000, target_q_paths=30000, train=True)
    a.checkpoint_save(str(tmp_path))
    d = make()
    d.checkpoint_load(str(tmp_path))
    for x, y in zip(d.get_subspace(), a.get_subspace()):
        assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()
    for x in (a, d):
        x.clear_accum()
        for f in range(2):
            x.render_frame("SPCBPT_eye", f)
        x.sync()
    assert np.array_equal(a.read_accum(), d.read_accum())
    # an environment map on top: ENV stays the last light, the mesh light's patches move up by 100, the films stay finite
    before = d.light_info()
    d.set_environment(pkg.scenes.sky_texture())
    info = d.light_info()
    assert [x["type"] for x in info] == [2, 1] and info[0]["first_subspace"] == before[0]["first_subspace"] - 100
    d.set_subspace()
    d.clear_accum()
    for alg in ("pt", "SPCBPT_eye"):
        for f in range(2):
            d.render_frame(alg, f)
        d.sync()
        img = d.read_accum()
        assert np.isfinite(img).all() and img[..., :3].mean() > 0
    v = d.lvc_read()
    o = v[v["depth"] == 0]
    assert set(np.unique(o["material_id"])) == {0, 1}


def test_render_tool_lights_a_gltf_file_by_its_emissive_meshes(sphere_room, pkg):
    """tools/spcbpt_render --emissive on the glTF file (which holds no quad): the PFM it writes is the film of the same frame
    sequence driven through ctypes; without the switch the file has no light and the tool says so."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run(["make", "-C", os.path.join(root, "tools"), "spcbpt_render"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    path = os.path.join(str(sphere_room["dir"]), "sphere_room.gltf")
    w, h, frames = 64, 48, 3
    out = os.path.join(str(sphere_room["dir"]), "tool")
    cmd = [os.path.join(root, "tools", "spcbpt_render"), path, ".", "--alg", "SPCBPT_eye", "--minimal", f"--dim={w}x{h}", "--frames", str(frames), "--out", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 1 and "quad light" in r.stdout, r.stdout
    r = subprocess.run(cmd + ["--emissive"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "mesh light 0: material 3, 320 triangles" in r.stdout, r.stdout
    raw = open(out + ".pfm", "rb").read()
    head = raw.split(b"\n", 3)
    assert head[0] == b"PF" and head[1] == f"{w} {h}".encode()
    tool = np.frombuffer(head[3], np.float32).reshape(h, w, 3)
    scene, _ = pkg.load_gltf(path, emissive=True)
    c = pkg.Renderer(scene, 0)
    cam = scene.camera
    c.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
    c.resize(w, h)
    c.set_light_trace(100000, 52, 1, 0, 0, True)                           # the tool's light pass
    c.set_subspace()
    for f in range(frames):
        c.launch("light trace", 1000001 + f); c.build_sampler(); c.launch("SPCBPT_eye", f)
    c.sync()
    film = c.read_accum()[..., :3]
    assert film.mean() > 0
    assert np.array_equal(tool, film)


# ------------------------------------------------------------------------------------------------------------ 10
def test_errors(gpu, pkg, hip_lib):
    def create(scene, lights):
        sd, keep = scene.desc()
        ml = (pkg.api.MeshLight * max(1, len(lights)))()
        for k, (mat, patches) in enumerate(lights):
            ml[k].material = mat; ml[k].emission[:] = [1.0, 1.0, 1.0]; ml[k].n_patches = patches
        h = C.c_void_p()
        rc = hip_lib.spcbpt_create_lit(C.byref(sd), ml, len(lights), 0, C.byref(h))
        msg = hip_lib.spcbpt_last_error(None).decode()
        if rc == 0:
            hip_lib.spcbpt_destroy(h)
        else:
            assert not h.value                  # no context leaks out of a failed create
        return rc, msg
    lamp = pkg.scenes.lamp_floor()
    assert create(lamp, [(1, 4)])[0] == 0
    for lights, text in (([], "light"), ([(2, 4)], "out of range"), ([(-1, 4)], "out of range"), ([(1, 4), (1, 4)], "twice"),
                         ([(1, 0)], "n_patches"), ([(1, 201)], "200"), ([(0, 150), (1, 51)], "200")):
        rc, msg = create(lamp, lights)
        assert rc == -1 and text in msg, (lights, rc, msg)
    unused = pkg.scenes.lamp_floor()
    unused.materials.append(dict(color=(1, 1, 1)))
    rc, msg = create(unused, [(2, 4)])
    assert rc == -1 and "no triangle" in msg
    flat = pkg.scenes.lamp_floor()
    flat.vertices = flat.vertices.copy()
    flat.vertices[np.unique(flat.indices[flat.tri_material == 1])] = (0.0, 1.5, 0.0)     # every lamp triangle collapses to a point
    rc, msg = create(flat, [(1, 4)])
    assert rc == -1 and "degenerate mesh light" in msg
    # quads and mesh lights share the patch budget
    both = pkg.scenes.lamp_floor()
    both.lights = [dict(position=(-2.0, 3.0, -2.0), u=(1.0, 0, 0), v=(0, 0, 1.0), emission=(5, 5, 5), div_level=14)]
    assert create(both, [(1, 4)])[0] == 0 and create(both, [(1, 5)])[0] == -1
    # spcbpt_create itself still wants a quad, in its own words
    sd, keep = lamp.desc()
    h = C.c_void_p()
    assert hip_lib.spcbpt_create(C.byref(sd), 0, C.byref(h)) == -1 and "quad light" in hip_lib.spcbpt_last_error(None).decode()
    # with an environment map the emitters may hold at most 100 patches; a light index out of range is an error
    rb = pkg.Renderer(pkg.scenes.cornell_sphere_lamp(n_patches=120), 0)
    with pytest.raises(pkg.SpcbptError):
        rb.set_environment(pkg.scenes.sky_texture())
    assert len(rb.light_info()) == 1
    assert hip_lib.spcbpt_light_info(rb.h, 1, None, None, None, None, None) == -1 and hip_lib.spcbpt_light_info(rb.h, -1, None, None, None, None, None) == -1
