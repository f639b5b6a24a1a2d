"""Seeded ray families for the float64 verdict (tests/ray_verdict.py): the rays a Gaussian direction from free space never produces.

Every family is 1024 rays [o, tmin = 1e-3, d, tmax] of float32 with unit directions; origins are uniform in the scene box shrunk by 0.05
unless stated.  tmax is 1e16 except for `shadow`.  Beside the rays each family carries a float32 `length` per ray: the length a pooled
shadow ray along it is given, and tmax_any = length - 1e-3 (formed in float32, as the pooled pass forms it) is the interval of its any-hit
runs -- for `shadow` that is the ray's own tmax, for the others a seeded length in [0.05, 4).

  random    Gaussian directions
  axis      direction +-e_k; the zero components are randomly +0.0 or -0.0
  planar    Gaussian direction with one exact zero component
  interior  aimed at a Dirichlet-random interior point of a random triangle
  vertex    aimed at a random triangle's P0
  edge      aimed at the midpoint of P0 P1
  surface   origin = the float32-rounded interior point; uniform direction
  shadow    origin as in `surface`, towards another such point; tmax = length - 1e-3; only pairs longer than 0.01 whose direction is at
            least 0.05 off both triangles' planes (|n^.d^| > 0.05): no coplanar rays
  outside   origin 50 units from the box centre, aimed at an interior point
"""
import zlib

import numpy as np

FAMILIES = ("random", "axis", "planar", "interior", "vertex", "edge", "surface", "shadow", "outside")
N = 1024
TMIN = np.float32(1e-3)
KEPS = np.float32(1e-3)   # SPCBPT_SCENE_EPSILON


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _interior(rng, P, n):
    """(points float32 (n, 3), triangle index): Dirichlet-random interior points of random triangles, rounded to float32"""
    k = rng.integers(0, len(P), n)
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    return (w[:, :, None] * P[k]).sum(1).astype(np.float32), k


def _pack(o, d, tmax, length):
    n = len(o)
    d32 = np.asarray(d, dtype=np.float32)
    rays = np.concatenate([np.asarray(o, dtype=np.float32), np.full((n, 1), TMIN, np.float32), d32, np.asarray(tmax, dtype=np.float32).reshape(n, 1)], 1)
    length = np.asarray(length, dtype=np.float32)
    return dict(rays=np.ascontiguousarray(rays), length=length, tmax_any=(length - KEPS).astype(np.float32))


def family(name, scene_name, P, lo, hi, n=N):
    """P: the verdict's triangles (float64 (T, 3, 3)); lo, hi: the scene box."""
    rng = np.random.default_rng(zlib.crc32(f"{scene_name}/{name}".encode()))
    lo, hi = np.asarray(lo, dtype=np.float64) + 0.05, np.asarray(hi, dtype=np.float64) - 0.05
    o = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    length = rng.uniform(0.05, 4.0, n).astype(np.float32)
    inf = np.full(n, 1e16, np.float32)
    if name == "random":
        return _pack(o, _unit(rng.normal(size=(n, 3))), inf, length)
    if name == "axis":
        d = np.where(rng.integers(0, 2, (n, 3)) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        d[np.arange(n), rng.integers(0, 3, n)] = np.where(rng.integers(0, 2, n) == 1, np.float32(-1.0), np.float32(1.0))
        return _pack(o, d, inf, length)
    if name == "planar":
        g = rng.normal(size=(n, 3))
        g[np.arange(n), rng.integers(0, 3, n)] = 0.0
        return _pack(o, _unit(g), inf, length)
    if name in ("interior", "vertex", "edge"):
        if name == "interior":
            target, _ = _interior(rng, P, n)
        else:
            k = rng.integers(0, len(P), n)
            target = P[k, 0] if name == "vertex" else 0.5 * (P[k, 0] + P[k, 1])
        return _pack(o, _unit(np.asarray(target, dtype=np.float64) - o.astype(np.float64)), inf, length)
    if name == "surface":
        s, _ = _interior(rng, P, n)
        return _pack(s, _unit(rng.normal(size=(n, 3))), inf, length)
    if name == "outside":
        centre = 0.5 * (lo + hi)
        s = (centre + 50.0 * _unit(rng.normal(size=(n, 3)))).astype(np.float32)
        target, _ = _interior(rng, P, n)
        return _pack(s, _unit(target.astype(np.float64) - s.astype(np.float64)), inf, length)
    if name == "shadow":
        e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        nh = np.cross(e1, e2)
        with np.errstate(invalid="ignore", divide="ignore"):   # (a zero-area triangle has no normal: its pairs fail the |n^.d^| test below)
            nh = nh / np.linalg.norm(nh, axis=1, keepdims=True)
        os_, ds_, ls_ = [], [], []
        have = 0
        for _ in range(64):
            a, ka = _interior(rng, P, 4 * n)
            b, kb = _interior(rng, P, 4 * n)
            v = b.astype(np.float64) - a.astype(np.float64)
            ln = np.linalg.norm(v, axis=1)
            with np.errstate(invalid="ignore", divide="ignore"):
                d = (v / ln[:, None]).astype(np.float32)
                dh = d.astype(np.float64)
                dh = dh / np.linalg.norm(dh, axis=1, keepdims=True)
                keep = (ln > 0.01) & (np.abs((nh[ka] * dh).sum(1)) > 0.05) & (np.abs((nh[kb] * dh).sum(1)) > 0.05)
            os_.append(a[keep]); ds_.append(d[keep]); ls_.append(ln[keep].astype(np.float32))
            have += int(keep.sum())
            if have >= n:
                break
        o2, d2, l2 = np.concatenate(os_)[:n], np.concatenate(ds_)[:n], np.concatenate(ls_)[:n]
        assert len(o2) == n, "shadow family: too few admissible pairs"
        tmax = (l2 - KEPS).astype(np.float32)
        return _pack(o2, d2, tmax, l2)
    raise ValueError(name)


SCENES = (("cornell_box", {}), ("simple_room", {"n": 6}), ("needle_room", {"n_needles": 2000}), ("bedroom", {"target_tris": 5000, "tex_size": 16}))


_BUILT = {}


def build_scene_cases(pkg, scene_name, kw, families=FAMILIES):
    """scene, verdict and, per family, the rays with their float64 table: built once per scene and session, shared by every entry point
    and never written to."""
    key = (scene_name, tuple(sorted(kw.items())), tuple(families))
    if key not in _BUILT:
        _BUILT[key] = _build(pkg, scene_name, kw, families)
    return _BUILT[key]


def _build(pkg, scene_name, kw, families):
    from tests import ray_verdict as rv
    scene = getattr(pkg.scenes, scene_name)(**kw)
    P, culled, ids = rv.scene_triangles(scene)
    V = rv.Verdict(P, culled)
    lo, hi = scene.vertices.min(0), scene.vertices.max(0)
    cases = {}
    for f in families:
        fam = family(f, scene_name, P, lo, hi)
        fam["table"] = V.table(fam["rays"], fam["tmax_any"])
        cases[f] = fam
    return dict(scene=scene, verdict=V, ids=ids, cases=cases, name=scene_name)
