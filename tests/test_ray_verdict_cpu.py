"""The float64 all-triangles verdict (tests/ray_verdict.py) held to the reference before it judges the device.

(a) The CPU oracle's closest-hit and any-hit answers over every (scene, family) of tests/ray_families.py: ZERO unexplained answers.
    Measured with K = 64, KT = 16: none over the 36 combinations; the oracle's worst |dt| / tt is 0.044 (bedroom, `edge`), so KT leaves
    it more than 20 x headroom; its smallest clear margin dist|cos| / dw among unambiguous rays is 1.00 (the definition's floor).
(b) Caps on the INPUTS: the share of ambiguous rays (more than one acceptable answer) is at most 2 % for `random`, `axis`, `planar`,
    `interior` on the furniture scenes and 8 % in the needle room (measured: at most 1.7 % / 7.5 %); every (scene, family) keeps at
    least 100 unambiguous rays (the smallest: needle-room `shadow`, 176).
(c) Seeded corruptions of the oracle's answers, each flagged on >= 99 % of the unambiguous rays it touches: the second-nearest clear hit
    for the nearest, a hit turned into a miss, t moved by 4 tt either way, a non-adjacent triangle, a culled emitter back face
    reported, visibility flipped.
"""
import os
import re

import numpy as np
import pytest

from tests import ray_families as rf
from tests import ray_verdict as rv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FURNITURE_CAP, NEEDLE_CAP, FLOOR = 0.02, 0.08, 100
CAPPED = ("random", "axis", "planar", "interior")


@pytest.fixture(scope="module", params=rf.SCENES, ids=[s[0] for s in rf.SCENES])
def sc(request, pkg, ob):
    name, kw = request.param
    c = rf.build_scene_cases(pkg, name, kw)
    o = ob.Oracle(c["scene"])
    ans = {}
    for f, fam in c["cases"].items():
        t, tri, _ = o.trace_closest(fam["rays"])
        ra = fam["rays"].copy()
        ra[:, 7] = fam["tmax_any"]
        ans[f] = dict(t=t, tri=tri, vis=o.trace_any(ra))
    return dict(c, oracle=o, answers=ans)


def test_oracle_answers_are_all_explained(sc):
    V = sc["verdict"]
    bad = []
    for f, fam in sc["cases"].items():
        a = sc["answers"][f]
        j = V.judge_closest(fam["table"], a["tri"], a["t"])
        ja = V.judge_any(fam["table"], a["vis"])
        amb, worst, margin = rv.report(j)
        print(f"{sc['name']:12s} {f:9s} ambiguous {amb:.4f} any-ambiguous {ja['ambiguous'].mean():.4f} worst |dt|/tt {worst:.3f} smallest clear margin {margin:.2f} "
              f"unexplained {int(j['unexplained'].sum())} / {int(ja['unexplained'].sum())}")
        if j["unexplained"].any() or ja["unexplained"].any():
            bad.append((f, np.nonzero(j["unexplained"])[0][:4].tolist(), np.nonzero(ja["unexplained"])[0][:4].tolist()))
    assert not bad, bad


def test_ambiguous_share_is_capped_and_enough_rays_are_left(sc):
    cap = NEEDLE_CAP if sc["name"] == "needle_room" else FURNITURE_CAP
    for f, fam in sc["cases"].items():
        amb = fam["table"]["closest"]["ambiguous"]
        if f in CAPPED:
            assert amb.mean() <= cap, (sc["name"], f, amb.mean())
        assert (~amb).sum() >= FLOOR, (sc["name"], f, int((~amb).sum()))
        assert (~fam["table"]["any"]["ambiguous_any"]).sum() >= FLOOR, (sc["name"], f)
        if f == "shadow":   # the construction keeps coplanar rays out
            assert fam["table"]["closest"]["coplanar"].mean() <= 0.01, (sc["name"], fam["table"]["closest"]["coplanar"].sum())


def _adjacent(P):
    """adjacency by POSITION (grids repeat corner positions under other vertex numbers): triangle -> set of triangles sharing a corner"""
    key = {}
    for i, tri in enumerate(P):
        for v in tri:
            key.setdefault(v.tobytes(), set()).add(i)
    return [set().union(*(key[v.tobytes()] for v in tri)) for tri in P]


def seeded_corruptions(sc):
    """(touched, flagged) per kind of corruption: the unambiguous rays each one changes, and how many of those the verdict then rejects"""
    V = sc["verdict"]
    rng = np.random.default_rng(99)
    adj = _adjacent(V.P)
    touched = {k: 0 for k in ("second", "miss", "t_plus", "t_minus", "triangle", "visibility")}
    flagged = dict(touched)
    for f, fam in sc["cases"].items():
        a, tab = sc["answers"][f], fam["table"]
        S = tab["closest"]
        un = ~S["ambiguous"]
        assert V.judge_closest(tab, a["tri"], a["t"])["ok"][un].all()
        # the second-nearest clear hit instead of the nearest
        m = un & (S["tri2"] >= 0)
        j = V.judge_closest(tab, np.where(m, S["tri2"], a["tri"]), np.where(m, S["t2"], a["t"]))
        touched["second"] += int(m.sum()); flagged["second"] += int((~j["ok"])[m].sum())
        # a hit turned into a miss
        m = un & (a["tri"] >= 0)
        j = V.judge_closest(tab, np.where(m, -1, a["tri"]), a["t"])
        touched["miss"] += int(m.sum()); flagged["miss"] += int((~j["ok"])[m].sum())
        # t scaled by 1 +- 4 tt / t
        idx = np.nonzero(m)[0]
        _, tt, _ = V.pair(fam["rays"][idx], a["tri"][idx])
        for name, sgn in (("t_plus", 1.0), ("t_minus", -1.0)):
            t2 = a["t"].astype(np.float64).copy()
            t2[idx] = t2[idx] * (1.0 + sgn * 4.0 * tt / t2[idx])
            j = V.judge_closest(tab, a["tri"], t2.astype(np.float32))
            touched[name] += len(idx); flagged[name] += int((~j["ok"])[idx].sum())
        # the triangle index replaced by a non-adjacent one
        tri2 = a["tri"].copy()
        for i in idx:
            while True:
                k = int(rng.integers(0, V.T))
                if k not in adj[int(a["tri"][i])]:
                    break
            tri2[i] = k
        j = V.judge_closest(tab, tri2, a["t"])
        touched["triangle"] += len(idx); flagged["triangle"] += int((~j["ok"])[idx].sum())
        # visibility flipped
        m = ~tab["any"]["ambiguous_any"]
        assert V.judge_any(tab, a["vis"])["ok"][m].all()
        j = V.judge_any(tab, 1 - a["vis"])
        touched["visibility"] += int(m.sum()); flagged["visibility"] += int((~j["ok"])[m].sum())
    return touched, flagged


def test_seeded_corruptions_are_flagged(sc):
    touched, flagged = seeded_corruptions(sc)
    for k in touched:
        print(sc["name"], k, flagged[k], "/", touched[k])
        assert touched[k] >= 500 and flagged[k] >= 0.99 * touched[k], (sc["name"], k, flagged[k], touched[k])


def test_a_culled_emitter_back_face_is_flagged(sc):
    """Rays that start 1.5 mm behind a quad light and cross it from the back: the oracle passes through (single-sided emitters), and the
    answer "the emitter" is not acceptable."""
    V, scene = sc["verdict"], sc["scene"]
    rng = np.random.default_rng(5)
    n_scene = len(scene.indices)
    n = 256
    k = n_scene + rng.integers(0, V.T - n_scene, n)
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    p = (w[:, :, None] * V.P[k]).sum(1)
    o = (p - 0.0015 * V.nhat[k] + rng.uniform(-0.0005, 0.0005, (n, 3))).astype(np.float32)
    d = p - o.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, np.full((n, 1), 1e-4, np.float32), d.astype(np.float32), np.full((n, 1), 1e16, np.float32)], 1)
    tab = V.table(rays)
    t, tri, _ = sc["oracle"].trace_closest(rays)
    j = V.judge_closest(tab, tri, t)
    assert not j["unexplained"].any()
    assert (tri < n_scene).all()                     # the oracle culls them all
    tk, _, _ = V.pair(rays, k)
    un = ~tab["closest"]["ambiguous"]
    jc = V.judge_closest(tab, k, tk.astype(np.float32))
    assert un.sum() >= 100 and (~jc["ok"])[un].mean() >= 0.99, (int(un.sum()), (~jc["ok"])[un].mean())
    # ... while any-hit rays see the emitter from both sides
    ra = rays.copy()
    ra[:, 7] = 0.01
    ta = V.table(ra)
    vis = sc["oracle"].trace_any(ra)
    assert not V.judge_any(ta, vis)["unexplained"].any() and (vis == 0).mean() > 0.9


def test_the_pooled_entry_point_copies_the_eye_kernels_constants():
    """csrc/pool_trace.hip runs trace_pool in the eye megakernel's frame: block size, resident blocks and hot-node count are the same text."""
    csrc = os.path.join(ROOT, "spcbpt-optix7_amd", "csrc")
    a, b = (open(os.path.join(csrc, f)).read() for f in ("kernels.hip", "pool_trace.hip"))
    for pat in (r"#define SPC_EYE_BLOCK \d+", r"#define SPC_EYE_WAVES \d+", r"static constexpr int EYE_BLOCK = [^;]+;", r"static constexpr int EYE_HOT = [^;]+;"):
        ma, mb = re.findall(pat, a), re.findall(pat, b)
        assert len(ma) == 1 and ma == mb, (pat, ma, mb)
    assert "__launch_bounds__(EYE_BLOCK, SPC_EYE_WAVES) void k_debug_trace_pool" in b
