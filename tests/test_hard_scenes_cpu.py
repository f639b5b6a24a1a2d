"""tests/test_ray_verdict_cpu.py's treatment for the hostile scenes of tests/hard_scenes.py, all without a GPU.

(a) The CPU oracle's closest-hit and any-hit answers on every scene and family: ZERO unexplained answers, K = 64 and KT = 16 unchanged.
(b) The seeded corruptions of tests/test_ray_verdict_cpu.py on the oracle's answers on far_4096, flat and duplicates: all flagged
    (every kind on >= 99 % of at least 500 unambiguous rays; `flat` has no second-nearest hits to swap in).
(c) Two conditions that keep the GPU test from passing vacuously, on the families `random`, `interior`, `surface`, `shadow`, `outside`:
    at most 15 % of the rays are ambiguous, at least 40 % have a clear hit.  `vertex`, `edge`, `axis`, `planar` aim at ambiguity by
    construction: they are run, printed and held to zero unexplained only.  A `shadow` ray ends 1e-3 before the surface point it aims
    at, so over its own interval it has a clear hit only where something occludes it; the pooled pass traces the same ray as an own ray
    over (1e-3, 1e16) too (the table's "open" summary), and that interval is the one counted here -- the share over the ray's own interval
    is printed beside it.
(d) The trees: tiny_k holds LEAF_MAX - 1, LEAF_MAX, LEAF_MAX + 1 triangles and leaves the SAH root with two and with three used slots,
    read from the built tree; nested is deeper than the LDS part of the stack (3 x depth > 16), and no ray of tools/bvh_eval.cpp's CPU
    traversal holds more than the 3 x depth entries that LDS + spill area give a lane (ctx_state.hip: spill_entries_needed).
(e) A zero-area triangle is never an acceptable answer.

Measured shares, ambiguous / clear hit in % (K = 64, KT = 16; the oracle's unexplained answers: 0 everywhere):
    scene            random      interior    surface     shadow      outside     axis        planar      vertex      edge
    tiny_1           0 / 49      0 / 99      1 / 17 *    0 / 100     0 / 73      0 / 29      0 / 43      77 / 22     82 / 17
    tiny_2           0 / 42      0 / 91      1 / 44      0 / 100     1 / 98      0 / 17      0 / 34      54 / 23     55 / 46
    tiny_3           0 / 47      0 / 95      1 / 52      0 / 100     0 / 99      0 / 18      0 / 31      45 / 39     47 / 55
    tiny_4           0 / 52      0 / 94      1 / 58      0 / 100     0 / 99      0 / 19      0 / 37      41 / 48     44 / 60
    tiny_5           0 / 54      0 / 96      1 / 63      0 / 100     1 / 98      0 / 21      0 / 37      32 / 60     35 / 67
    flat             0 / 44      4 / 96      1 / 0 *     -           3 / 96      0 / 17      0 / 31      100 / 0     100 / 0
    far_64           0 / 85      1 / 100     10 / 78     3 / 100     1 / 100     0 / 86      0 / 85      60 / 78     46 / 82
    far_256          3 / 84      9 / 98      68 / 76 *   64 / 99 *   5 / 99      3 / 85      3 / 87      65 / 72     54 / 77
    far_4096         45 / 63 *   74 / 76 *   100 / 53 *  100 / 77 *  44 / 83 *   42 / 75     43 / 69     88 / 54     84 / 62
    far_tiles        2 / 98      3 / 97      12 / 50     5 / 97      6 / 99      2 / 98      1 / 99      100 / 0     100 / 0
    far_tiles_256    14 / 86     22 / 78 *   72 / 41 *   59 / 80 *   28 / 91 *   7 / 93      14 / 86     100 / 0     100 / 0
    duplicates       0 / 100     0 / 100     1 / 99      0 / 100     0 / 100     0 / 100     0 / 100     46 / 99     41 / 99
    mixed_scale      0 / 42      13 / 98     4 / 63      5 / 99      11 / 99     0 / 17      0 / 31      77 / 78     75 / 80
    mixed_scale_2000 0 / 49      76 / 82 *   100 / 58 *  100 / 78 *  35 / 99 *   0 / 18      0 / 35      87 / 74     86 / 74
    nested           0 / 100     5 / 100     2 / 95      2 / 100     0 / 100     0 / 100     0 / 100     54 / 91     46 / 92
    nested_08        0 / 100     58 / 100 *  33 / 93 *   46 / 100 *  0 / 100     0 / 100     0 / 100     85 / 92     85 / 92
(* = listed in hard_scenes.UNCAPPED with its reason, and asserted here to miss the caps; `flat` has no `shadow` family.)  A `shadow` ray's
clear hits over its OWN interval, i.e. occluded rays: tiny_1 0, tiny_2 0, tiny_3 55, tiny_4 63, tiny_5 68, far_64 55, far_256 52, far_4096 17,
far_tiles 0, far_tiles_256 0, duplicates 64, mixed_scale 15, mixed_scale_2000 9, nested 83, nested_08 52 %.
The oracle's worst |dt| / tt over all scenes and families is 0.057 (mixed_scale, `outside`); its smallest clear margin 1.00.
What the scenes' parameters had to give for the caps: the Cornell box and the tiles are held to all five families at an offset of
(32, -16, 64) -- beyond about 100 units a ray that leaves a surface cannot be told from one that re-meets it (tt ~ 1e-6 ext / |cos| against
tmin = 1e-3) -- and to `random`, `interior`, `outside` (Cornell box) at (256, -128, 512); the tiles have four walls and the light as their
ceiling (with two walls `surface` had 17 % clear hits); mixed_scale has a 40-unit ground quad and small triangles of 0.03 - 0.1 (the
`outside` rays' dw ~ 4e-4 alone is a fifth of a 0.01 - 0.05 triangle); nested falls by 0.95 per triangle; duplicates and nested stand in a
closed room; the grid of `flat` is 8 units wide.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import hard_scenes as hs
from tests import ray_verdict as rv
from tests import test_ray_verdict_cpu as base

AMBIGUOUS_CAP, CLEAR_FLOOR = 0.15, 0.40
CAPPED = ("random", "interior", "surface", "shadow", "outside")


@pytest.fixture(scope="module", params=hs.HARD_SCENES, ids=[s[0] for s in hs.HARD_SCENES])
def sc(request, pkg, ob):
    name, kw = request.param
    c = hs.build_scene_cases(pkg, name, kw)
    o = ob.Oracle(c["scene"])
    ans = {}
    for f, fam in c["cases"].items():
        t, tri, _ = o.trace_closest(fam["rays"])
        ra = fam["rays"].copy()
        ra[:, 7] = fam["tmax_any"]
        ans[f] = dict(t=t, tri=tri, vis=o.trace_any(ra))
    return dict(c, oracle=o, answers=ans)


def test_oracle_answers_are_all_explained(sc):
    base.test_oracle_answers_are_all_explained(sc)


def test_the_rays_are_neither_mostly_ambiguous_nor_mostly_misses(sc):
    bad = []
    for f, fam in sc["cases"].items():
        amb = float(fam["table"]["open"]["ambiguous"].mean())
        clear = float(fam["table"]["open"]["has_clear"].mean())
        own = float(fam["table"]["closest"]["has_clear"].mean())
        print(f"{sc['name']:12s} {f:9s} ambiguous {100 * amb:5.1f} % clear hit {100 * clear:5.1f} % (own interval {100 * own:5.1f} %, any-hit ambiguous "
              f"{100 * fam['table']['any']['ambiguous_any'].mean():5.1f} %)")
        if f not in CAPPED:
            continue
        meets = amb <= AMBIGUOUS_CAP and clear >= CLEAR_FLOOR and float(fam["table"]["closest"]["ambiguous"].mean()) <= AMBIGUOUS_CAP
        beyond = f in hs.UNCAPPED.get(sc["name"], ())
        if meets == beyond:   # (hard_scenes.UNCAPPED lists what cannot meet the caps: a listed family that meets them is an error too)
            bad.append((f, amb, clear, "listed as uncapped" if beyond else "misses the caps"))
        assert (~fam["table"]["open"]["ambiguous"]).sum() >= 100 or beyond, (sc["name"], f)
    assert not bad, (sc["name"], bad)


def test_seeded_corruptions_are_flagged(sc):
    """The bars of tests/test_ray_verdict_cpu.py: every kind touches at least 500 unambiguous rays and is flagged on 99 % of them.  (One
    kind cannot exist in one scene: no ray meets the plane of `flat` twice, so no ray there has a second-nearest clear hit.)"""
    if sc["name"] not in ("far_4096", "flat", "duplicates"):
        return
    touched, flagged = base.seeded_corruptions(sc)
    for k in touched:
        print(sc["name"], k, flagged[k], "/", touched[k])
        if sc["name"] == "flat" and k == "second":
            assert touched[k] == 0
            continue
        assert touched[k] >= 500 and flagged[k] >= 0.99 * touched[k], (sc["name"], k, flagged[k], touched[k])


def test_a_zero_area_triangle_is_never_an_answer(pkg):
    c = hs.build_scene_cases(pkg, "duplicates", {})
    V = c["verdict"]
    zero = np.nonzero(V.degenerate)[0]
    assert len(zero) == 32 and (np.bincount(V.group) == 9).sum() == 64   # 64 triangles nine times each, bit for bit
    fam = c["cases"]["interior"]
    n = len(fam["rays"])
    for k in zero[:8]:
        t, _, _ = V.pair(fam["rays"], np.full(n, k))
        j = V.judge_closest(fam["table"], np.full(n, k), np.nan_to_num(t).astype(np.float32))
        assert not j["ok"].any()
        assert (j["unexplained"] | fam["table"]["closest"]["coplanar"]).all()


def test_the_trees_are_the_ones_the_scenes_are_named_for(pkg):
    info = {}
    for name, kw in hs.HARD_SCENES:
        if name.startswith("tiny_") or name in ("nested", "flat"):
            P, _, _ = rv.scene_triangles(hs.make(pkg, name, kw))
            info[name] = dict(hs.tree_info(P), T=len(P))
            print(name, info[name])
    L = hs.LEAF_MAX
    assert [info[f"tiny_{k}"]["T"] for k in hs.TINY_KS[:3]] == [L - 1, L, L + 1]
    assert [info[f"tiny_{k}"]["root_slots"] for k in hs.TINY_KS] == [1, 1, 2, 2, 3], info
    assert info[f"tiny_{hs.TINY_KS[1]}"]["nodes"] == 1 and info[f"tiny_{hs.TINY_KS[1]}"]["leaves"] == 1      # the n <= LEAF_MAX root: one real leaf
    assert 3 * info["nested"]["depth"] > 16, info["nested"]


@pytest.mark.parametrize("name", ["nested", "nested_08"])
def test_no_ray_of_the_cpu_traversal_outgrows_the_stack_of_nested(pkg, tmp_path, name):
    """TravStack holds 16 entries in LDS and 3 x bvh_depth - 16 in HBM per thread (ctx_state.hip: spill_entries_needed; the area is
    sized per launched thread by ensure_spill): 3 x depth in all.  tools/bvh_eval.cpp's traversal pushes what the device pushes: over
    its own rays and over every family's (closest-hit and any-hit) no stack outgrows that, and some family does go past the LDS part --
    the GPU test's "the spill area was written" has rays that write it.  Measured deepest stacks: nested 23 of 27, nested_08 52 of 57."""
    exe = str(tmp_path / "bvh_eval")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(hs.ROOT, "tools", "bvh_eval.cpp")], check=True)
    c = hs.build_scene_cases(pkg, name, dict(hs.HARD_SCENES)[name])
    mesh, rays = str(tmp_path / "mesh.bin"), str(tmp_path / "rays.bin")
    hs.write_mesh(mesh, c["verdict"].P)
    bound = 3 * hs.tree_info(c["verdict"].P)["depth"]
    assert bound > 16
    deepest = {}
    for f, fam in c["cases"].items():
        fam["rays"].tofile(rays)
        r = subprocess.run([exe, mesh, "2000", rays], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        found = re.findall(r"deepest stack of a ray: (\d+) entries \(3 x depth = (\d+)\)", r.stdout)
        assert len(found) == 2 and all(int(b) == bound for _, b in found), r.stdout
        deepest[f] = int(found[0][0])
        assert 0 < int(found[1][0]) <= bound, r.stdout
    print(name, bound, deepest)
    assert max(deepest.values()) <= bound and max(deepest.values()) > 16, (bound, deepest)
