"""Every traversal path of the device, the POOLED pass of the eye megakernel included, judged ray by ray by the float64 all-triangles
verdict of tests/ray_verdict.py (held to the CPU oracle by tests/test_ray_verdict_cpu.py): every scene and ray family of
tests/ray_families.py, ZERO unexplained answers.

Entry points: trace_closest / trace_any (traverse<>: the light pass, pt, splat, features), trace_bench modes 0-4 (the pool-fed lane loop
and the quad-lane kernels), and trace_pool (csrc/pool_trace.hip: one pass of the megakernel's trace_pool) with 64 own rays and a full
pool per wave, own rays only, pool only, 5 own + 3 shadow rays per wave (straight into the quad tail) and a lane count that is no
multiple of 64 -- again on renderers created with SPCBPT_NO_FAN_TAIL=1 and with SPCBPT_BVH_HOT_NODES=0.  The pooled pass traces its own
rays over (1e-3, 1e16) and a shadow ray over (1e-3, length - 1e-3); the verdict is given those intervals.

Measured on an MI355X with K = 64, KT = 16 (neither was raised; the CPU oracle on the same rays in brackets, from
test_ray_verdict_cpu.py): unexplained answers 0 on every entry point, scene and family [0]; worst |dt| / tt among unambiguous hits 0.046
(bedroom `shadow` through trace_pool; 0.038 through traverse<> and trace_bench, needle-room `edge`) [0.044, bedroom `edge`]; smallest
clear margin dist|cos| / dw of an accepted unambiguous hit 1.00 [1.00] -- the definition's floor.  needle_room(2000): 3 x bvh_depth - 16
> 0 and the HBM spill area is written both by traverse<> and by the pooled pass.  Shared-edge leaks of 16 384 rays: Cornell box oracle
1 204, device 958 (every entry point); simple_room(6) oracle 1 038, device 1 108 (1 112 through trace_bench mode 4); bound 1.25 x + 30.
Each case prints its ambiguous share, worst |dt| / tt and smallest clear margin (pytest -s).
"""
import numpy as np
import pytest

from tests import ray_families as rf
from tests import ray_verdict as rv

pytestmark = pytest.mark.gpu

CONNECTION_N = 3


@pytest.fixture(scope="module", params=rf.SCENES, ids=[s[0] for s in rf.SCENES])
def sc(request, gpu, pkg):
    name, kw = request.param
    c = rf.build_scene_cases(pkg, name, kw)
    return dict(c, renderer=pkg.Renderer(c["scene"], 0))


def _line(sc, entry, f, j, ja=None):
    amb, worst, margin = rv.report(j) if j is not None else (float("nan"), 0.0, float("inf"))
    s = f"{sc['name']:12s} {entry:22s} {f:9s} ambiguous {amb:.4f} worst |dt|/tt {worst:.3f} smallest clear margin {margin:.2f}"
    if j is not None:
        s += f" unexplained {int(j['unexplained'].sum())}"
    if ja is not None:
        s += f" | any-hit ambiguous {ja['ambiguous'].mean():.4f} unexplained {int(ja['unexplained'].sum())}"
    print(s)


def _bad(tab, j, limit=3):
    """the first unexplained rays with their answers' context, for the failure message"""
    idx = np.nonzero(j["unexplained"])[0][:limit]
    return [(int(i), tab["rays"][i].tolist()) for i in idx]


def _any_rays(fam):
    ra = fam["rays"].copy()
    ra[:, 7] = fam["tmax_any"]
    return ra


def test_traverse_answers_are_all_explained(sc):
    V, r = sc["verdict"], sc["renderer"]
    bad = []
    needle = sc["name"] == "needle_room"
    if needle:
        assert 3 * r.scene_info()["bvh_depth"] - 16 > 0, r.scene_info()
        r.trace_closest(sc["cases"]["random"]["rays"])   # sizes the spill area
        r.spill_arm()
    for f, fam in sc["cases"].items():
        t, tri, _ = r.trace_closest(fam["rays"])
        vis = r.trace_any(_any_rays(fam))
        j, ja = V.judge_closest(fam["table"], tri, t), V.judge_any(fam["table"], vis)
        _line(sc, "traverse", f, j, ja)
        if j["unexplained"].any() or ja["unexplained"].any():
            bad.append((f, _bad(fam["table"], j), _bad(fam["table"], ja)))
    assert not bad, bad
    if needle:
        assert r.spill_count()[0] > 0, r.spill_count()


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_trace_bench_answers_are_all_explained(sc, pkg, mode):
    V, r = sc["verdict"], sc["renderer"]
    cap = {0: None, 1: 64, 2: 48, 3: 48, 4: 64}[mode]
    if cap is not None and 3 * r.scene_info()["bvh_depth"] > cap:
        # the quad kernels' per-ray LDS stack does not hold this BVH: the entry point must refuse, not answer
        with pytest.raises(pkg.SpcbptError):
            r.trace_bench(sc["cases"]["random"]["rays"], mode, False, repeat=1, stats=False)
        return
    bad = []
    for f, fam in sc["cases"].items():
        (t, tri, _), _, _ = r.trace_bench(fam["rays"], mode, False, repeat=1, stats=False)
        vis, _, _ = r.trace_bench(_any_rays(fam), mode, True, repeat=1, stats=False)
        j, ja = V.judge_closest(fam["table"], tri, t), V.judge_any(fam["table"], vis)
        _line(sc, f"trace_bench {mode}", f, j, ja)
        if j["unexplained"].any() or ja["unexplained"].any():
            bad.append((f, _bad(fam["table"], j), _bad(fam["table"], ja)))
    assert not bad, bad


# ---- the pooled pass ----------------------------------------------------------------------------------------------------------------
def _pool_inputs(fam, ray_of_lane, own, slots):
    """Lane i carries family ray ray_of_lane[i]: as its own ray where own[i], and -- with its length -- in every slot k where slots[i, k]."""
    rays = fam["rays"][ray_of_lane]
    sh = np.zeros((len(ray_of_lane), CONNECTION_N, 4), np.float32)
    sh[:, :, :3] = rays[:, None, 4:7]
    sh[:, :, 3] = np.where(slots, fam["length"][ray_of_lane][:, None], np.float32(-1.0))
    return rays, own.astype(np.int32), rays[:, 0:3], sh


PATTERNS = ("full", "own_only", "pool_only", "quad_tail", "ragged")


def _pattern(name, n_rays):
    if name in ("full", "own_only", "pool_only", "ragged"):
        n = n_rays - 24 if name == "ragged" else n_rays          # 1000 lanes: the last wave holds 40
        lane_ray = np.arange(n)
        own = np.full(n, name != "pool_only")
        slots = np.full((n, CONNECTION_N), name != "own_only")
        return lane_ray, own, slots
    # 5 own + 3 shadow rays per wave, at lanes and slots that move from wave to wave; 128 waves over the family's rays
    waves = 128
    n = waves * 64
    lane_ray = np.arange(n) % n_rays
    own = np.zeros(n, bool)
    slots = np.zeros((n, CONNECTION_N), bool)
    for w in range(waves):
        own[w * 64 + (7 * w + 13 * np.arange(5)) % 64] = True
        for k in range(3):
            slots[w * 64 + (11 * w + 29 * k + 5) % 64, (w + k) % CONNECTION_N] = True
    return lane_ray, own, slots


def _run_pool(sc, r, f, fam, pattern, entry, bad):
    V = sc["verdict"]
    lane_ray, own, slots = _pattern(pattern, len(fam["rays"]))
    own_rays, mask, org, sh = _pool_inputs(fam, lane_ray, own, slots)
    t, tri, _, length = r.trace_pool(own_rays, mask, org, sh)
    j = ja = None
    if own.any():
        sel = lane_ray[own]
        j = V.judge_closest(fam["table"], tri[own], t[own], which="open", sel=sel)
        if j["unexplained"].any():
            bad.append((f, pattern, "own", [(int(sel[i]), fam["rays"][sel[i]].tolist(), int(tri[own][i]), float(t[own][i])) for i in np.nonzero(j["unexplained"])[0][:3]]))
    assert (tri[~own] == -1).all(), (f, pattern)                       # a lane without an own ray reports no hit
    assert (length[~slots] == -1.0).all(), (f, pattern)                # an empty slot stays empty
    if slots.any():
        li, ki = np.nonzero(slots)
        out = length[li, ki]
        vis = (out >= 0).astype(np.int32)
        assert ((out == sh[li, ki, 3]) | (out == -1.0)).all(), (f, pattern)   # an unoccluded ray keeps its length, an occluded one reads -1
        sel = lane_ray[li]
        ja = V.judge_any(fam["table"], vis, sel=sel)
        if ja["unexplained"].any():
            bad.append((f, pattern, "shadow", [(int(sel[i]), fam["rays"][sel[i]].tolist(), float(fam["length"][sel[i]]), int(vis[i])) for i in np.nonzero(ja["unexplained"])[0][:3]]))
    _line(sc, f"{entry} {pattern}", f, j, ja)


def test_pooled_pass_answers_are_all_explained(sc):
    r = sc["renderer"]
    needle = sc["name"] == "needle_room"
    bad = []
    for pattern in PATTERNS:
        if needle and pattern == "full":
            fam = sc["cases"]["random"]
            r.trace_pool(*_pool_inputs(fam, *_pattern("full", len(fam["rays"]))))   # sizes the spill area
            r.spill_arm()
        for f, fam in sc["cases"].items():
            _run_pool(sc, r, f, fam, pattern, "trace_pool", bad)
        if needle and pattern == "full":
            assert r.spill_count()[0] > 0, r.spill_count()
    assert not bad, bad


@pytest.mark.parametrize("knob", ["SPCBPT_NO_FAN_TAIL", "SPCBPT_BVH_HOT_NODES"])
def test_pooled_pass_without_fan_tail_and_without_hot_order(sc, pkg, monkeypatch, knob):
    """The quad tail to its end without the fan-out tail; a BVH numbered depth-first throughout (the LDS hot-node table then holds other nodes)."""
    monkeypatch.setenv(knob, "1" if knob == "SPCBPT_NO_FAN_TAIL" else "0")
    r = pkg.Renderer(sc["scene"], 0)
    monkeypatch.delenv(knob)
    bad = []
    for pattern in ("full", "pool_only", "quad_tail"):
        for f, fam in sc["cases"].items():
            _run_pool(sc, r, f, fam, pattern, knob[7:].lower(), bad)
    assert not bad, bad


# ---- rays at shared edges: measured, and bounded by the reference ---------------------------------------------------------------
def _shared_edge_rays(scene, P, n, seed):
    """Rays aimed at interior points of edges that two of the scene's triangles share BY VERTEX INDEX, from 0.02-0.3 away on the front
    side of both, at least 0.2 off grazing to both faces.  Returns (rays, triangle A, triangle B, distance to the edge point)."""
    I = np.asarray(scene.indices, dtype=np.int64)
    owner = {}
    for ti, tri in enumerate(I):
        for a, b in ((0, 1), (1, 2), (2, 0)):
            owner.setdefault((min(tri[a], tri[b]), max(tri[a], tri[b])), []).append(ti)
    edges = np.array([(k[0], k[1], v[0], v[1]) for k, v in owner.items() if len(v) == 2], dtype=np.int64)
    assert len(edges) >= 8
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    nh = np.cross(e1, e2)
    nh /= np.linalg.norm(nh, axis=1, keepdims=True)
    Vx = np.asarray(scene.vertices, dtype=np.float64)
    rng = np.random.default_rng(seed)
    out = []
    have = 0
    while have < n:
        e = edges[rng.integers(0, len(edges), 2 * n)]
        s = rng.uniform(0.05, 0.95, (2 * n, 1))
        p = (1 - s) * Vx[e[:, 0]] + s * Vx[e[:, 1]]
        u = 0.5 * (nh[e[:, 2]] + nh[e[:, 3]]) + 0.7 * rng.normal(size=(2 * n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        keep = ((nh[e[:, 2]] * u).sum(1) >= 0.2) & ((nh[e[:, 3]] * u).sum(1) >= 0.2)
        o = (p + u * rng.uniform(0.02, 0.3, (2 * n, 1))).astype(np.float32)
        out.append((o[keep], p[keep], e[keep]))
        have += int(keep.sum())
    o = np.concatenate([x[0] for x in out])[:n]
    p = np.concatenate([x[1] for x in out])[:n]
    e = np.concatenate([x[2] for x in out])[:n]
    v = p - o.astype(np.float64)
    dist = np.linalg.norm(v, axis=1)
    d = (v / dist[:, None]).astype(np.float32)
    rays = np.concatenate([o, np.full((n, 1), 1e-3, np.float32), d, np.full((n, 1), 1e16, np.float32)], 1)
    return np.ascontiguousarray(rays), e[:, 2], e[:, 3], dist


def _leaks(tri, t, a, b, dist):
    """an answer that is neither of the two triangles nor clearly nearer than them"""
    nearer = (tri >= 0) & (t.astype(np.float64) < dist - 1e-4 * np.maximum(1.0, dist))
    return int((~((tri == a) | (tri == b) | nearer)).sum())


@pytest.mark.parametrize("scene_name", ["cornell_box", "simple_room"])
def test_shared_edge_leaks_are_no_more_than_the_references(gpu, pkg, ob, scene_name):
    """Float32 Moller-Trumbore is not watertight at an edge two triangles share: the CPU oracle itself leaks there.  The device may leak
    no more than 1.25 x the oracle on the same 16 384 rays, plus 30.  (This records the property; it does not fix it.)"""
    sc = rf.build_scene_cases(pkg, scene_name, dict(rf.SCENES)[scene_name])
    rays, a, b, dist = _shared_edge_rays(sc["scene"], sc["verdict"].P, 16384, 21)
    o = ob.Oracle(sc["scene"])
    t0, tri0, _ = o.trace_closest(rays)
    leak0 = _leaks(tri0, t0, a, b, dist)
    r = pkg.Renderer(sc["scene"], 0)
    n = len(rays)
    results = {"traverse": r.trace_closest(rays)[:2]}
    for mode in range(5):
        (t, tri, _), _, _ = r.trace_bench(rays, mode, False, repeat=1, stats=False)
        results[f"trace_bench {mode}"] = (t, tri)
    empty = np.full((n, CONNECTION_N, 4), -1.0, np.float32)
    t, tri, _, _ = r.trace_pool(rays, np.ones(n, np.int32), rays[:, :3], empty)
    results["trace_pool"] = (t, tri)
    print(f"{sc['name']}: shared-edge leaks of {n} rays: oracle {leak0}", {k: _leaks(v[1], v[0], a, b, dist) for k, v in results.items()})
    for k, (t, tri) in results.items():
        assert _leaks(tri, t, a, b, dist) <= 1.25 * leak0 + 30, (k, _leaks(tri, t, a, b, dist), leak0)
