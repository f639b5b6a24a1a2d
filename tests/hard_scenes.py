"""Seeded hostile scenes for the float64 verdict (tests/ray_verdict.py): the geometry that breaks BVH builders and quantised slab tests.

The four scenes of tests/ray_families.py sit at the origin, are a few units across and have thousands of well-shaped triangles.  These do
not.  Every scene has at most about 1 500 triangles and ONE quad light (every entry point can create a renderer on it):

  tiny_k       k large scene triangles closely over a 4 x 4 quad light that faces them: the BVH holds k + 2 triangles.  k = LEAF_MAX - 3,
               LEAF_MAX - 2, LEAF_MAX - 1 put LEAF_MAX - 1, LEAF_MAX and LEAF_MAX + 1 triangles into the tree (the `n <= LEAF_MAX` root with
               one leaf and one empty child, and the first real split); TINY_TWO_SLOTS and TINY_THREE_SLOTS leave the root of the SAH tree
               with exactly two and three used slots -- read from the built tree (tree_info) by tests/test_hard_scenes_cpu.py
  flat         a 16 x 16 grid of quads and the light, all with y exactly 0: every node has a zero-extent axis (exponent fallback e = 0)
  far_64       the Cornell box, every vertex and the light moved by (32, -16, 64): float32(float64(v) + T)
  far_256      ... by (256, -128, 512)
  far_4096     ... by (4096, -2048, 8192)
  far_tiles    a 12 x 12 floor of separate axis-aligned square tiles of edge 0.25 (flat leaf boxes), four walls of them and the light as the
               ceiling, moved by (32, -16, 64); far_tiles_256: by (256, -128, 512)
  duplicates   64 distinct triangles, each present 9 times bit for bit (more copies than a leaf holds: coinciding centroids), and 32
               zero-area triangles (two equal corners, three collinear corners, three equal corners), in a seeded order, in a closed room
  mixed_scale  the two triangles of a 40-unit ground quad, 300 triangles of 0.03 - 0.1 units inside a unit cube resting on it and 100
               triangles of about one unit around them; mixed_scale_2000: a ground quad of 2 000 units, triangles of 0.01 - 0.05
  nested       120 triangles whose sizes fall by a factor of 0.95 towards one corner, in a closed room: the SAH tree is a long chain, deeper
               than the LDS part of the traversal stack; nested_08: a factor of 0.8

The offsets, the ground quad and the factor of the first of each pair are the largest at which the verdict still decides most rays (the
caps of tests/test_hard_scenes_cpu.py); the second of each pair (UNCAPPED) is the geometry as users bring it, judged on the rays the
verdict can still decide.

The ray box of a scene is its bounding box (scene vertices and light corners) grown symmetrically to at least 1 unit on every axis:
ray_families.family shrinks the box it is given by 0.05, which a flat scene cannot give.
"""
import atexit
import os
import re
import shutil
import subprocess
import tempfile
import zlib

import numpy as np

from tests import ray_families as rf
from tests import ray_verdict as rv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def leaf_max():
    m = re.search(r"#define SPC_LEAF_MAX (\d+)", open(os.path.join(ROOT, "spcbpt-optix7_amd", "csrc", "layout.h")).read())
    return int(m.group(1))


LEAF_MAX = leaf_max()
TINY_TWO_SLOTS, TINY_THREE_SLOTS = 4, 5        # k: the SAH root then has two / three used slots (held to the built tree by the CPU test)
TINY_KS = (LEAF_MAX - 3, LEAF_MAX - 2, LEAF_MAX - 1, TINY_TWO_SLOTS, TINY_THREE_SLOTS)
FAR_64, FAR_256, FAR_4096 = (32.0, -16.0, 64.0), (256.0, -128.0, 512.0), (4096.0, -2048.0, 8192.0)

HARD_SCENES = tuple((f"tiny_{k}", {"k": k}) for k in TINY_KS) + (
    ("flat", {}),
    ("far_64", {"offset": FAR_64}), ("far_256", {"offset": FAR_256}), ("far_4096", {"offset": FAR_4096}),
    ("far_tiles", {"edge": 0.25, "offset": FAR_64}), ("far_tiles_256", {"edge": 0.25, "offset": FAR_256}),
    ("duplicates", {}),
    ("mixed_scale", {"ground": 40.0, "small": (0.03, 0.1)}), ("mixed_scale_2000", {"ground": 2000.0, "small": (0.01, 0.05)}),
    ("nested", {"factor": 0.95}), ("nested_08", {"factor": 0.8}))

# (scene, families) that the caps on the inputs (tests/test_hard_scenes_cpu.py: at most 15 % ambiguous rays, at least 40 % with a clear hit)
# cannot hold: run, printed and held to zero unexplained answers like every other.  The CPU test measures each and asserts that it does
# miss the caps, so nothing stays listed that need not be.
_OFF = ("interior", "surface", "shadow", "outside")
UNCAPPED = {
    # the verdict's own rounding bands swallow the rays:
    # a ray that leaves a surface re-meets it at t = 0, and whether (tmin = 1e-3) excludes that is decided by tt ~ 1e-6 ext / |cos|
    "far_256": ("surface", "shadow"),
    "far_tiles_256": _OFF,        # ... and dw = 64 x 2^-24 x (ext + |o| + t) ~ 0.004 against tiles of 0.25
    "far_4096": ("random",) + _OFF,   # dw ~ 0.06 in a box 2 units across
    "mixed_scale_2000": _OFF,     # dw ~ 0.008 against triangles of 0.01 - 0.05
    "nested_08": ("interior", "surface", "shadow"),   # two thirds of the triangles are smaller than dw
    # the geometry has no such rays:
    "tiny_1": ("surface",),       # two plane pieces see each other along at most half of all directions, and 2 of the 3 triangles are the light
    "flat": ("surface",),         # everything lies in one plane: a ray that leaves it meets nothing
}
# `flat` has no `shadow` family: every pair of its surface points lies in the one plane, and the family admits no coplanar ray
NO_FAMILY = {"flat": ("shadow",)}

_GREY = dict(color=(0.7, 0.7, 0.7), roughness=0.5, metallic=0.0)


def _scene(pkg, name, V, I, light):
    V = np.ascontiguousarray(V, dtype=np.float32).reshape(-1, 3)
    I = np.ascontiguousarray(I, dtype=np.uint32).reshape(-1, 3)
    lo, hi = V.min(0).astype(np.float64), V.max(0).astype(np.float64)
    c = 0.5 * (lo + hi)
    cam = dict(eye=tuple(c + np.array([0.0, 0.3, 1.5]) * max(1.0, float((hi - lo).max()))), lookat=tuple(c), up=(0, 1, 0), fov=40.0)
    return pkg.api.Scene(vertices=V, indices=I, tri_material=np.zeros(len(I), np.int32), materials=[dict(_GREY)], lights=[dict(light, div_level=2)],
                         texcoords=np.zeros((len(V), 2), np.float32), camera=cam, name=name)


def _soup(P):
    """(vertices, indices) of an unindexed triangle list (T, 3, 3)"""
    P = np.asarray(P, dtype=np.float32)
    return P.reshape(-1, 3), np.arange(3 * len(P), dtype=np.uint32).reshape(-1, 3)


def _rng(name):
    return np.random.default_rng(zlib.crc32(f"hard/{name}".encode()))


def tiny(pkg, k):
    """k large triangles above a 4 x 4 light that faces up.  One triangle: inside the light's footprint, 0.3 - 1 above it.  More: the
    first two are a roof quad closely over the light and the others lie in layers above it."""
    rng = _rng(f"tiny_{k}")
    P = np.zeros((k, 3, 3))
    sq = np.array([[-0.1, -0.1], [4.1, -0.1], [4.1, 4.1], [-0.1, 4.1]])
    if k == 1:
        P[0, :, 0], P[0, :, 2], P[0, :, 1] = (0.1, 3.9, 0.1), (0.1, 0.1, 3.9), rng.uniform(0.3, 1.0, 3)
    else:
        h = rng.uniform(0.03, 0.06, 4)
        for i, pick in enumerate(((0, 1, 2), (0, 2, 3))):
            P[i, :, 0], P[i, :, 2], P[i, :, 1] = sq[list(pick), 0], sq[list(pick), 1], h[list(pick)]
        for i in range(2, k):
            pick = list(np.roll(np.arange(4), i)[:3])
            P[i, :, 0], P[i, :, 2] = sq[pick, 0], sq[pick, 1]
            P[i, :, 1] = 0.1 * (i - 1) + rng.uniform(0.0, 0.03, 3)
    V, I = _soup(P)
    light = dict(position=(0.0, 0.0, 0.0), u=(0.0, 0.0, 4.0), v=(4.0, 0.0, 0.0), emission=(5, 5, 5))   # cross(u, v) = +y
    return _scene(pkg, f"tiny_{k}", V, I, light)


def _grid(p0, du, dv, nu, nv):
    """an indexed (nu x nv) grid of quads, two triangles each; float64 vertices"""
    p0, du, dv = (np.asarray(a, dtype=np.float64) for a in (p0, du, dv))
    S, T = np.meshgrid(np.arange(nu + 1) / nu, np.arange(nv + 1) / nv, indexing="ij")
    P = p0 + S[..., None] * du + T[..., None] * dv
    idx = np.arange((nu + 1) * (nv + 1)).reshape(nu + 1, nv + 1)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[1:, 1:], idx[:-1, 1:]
    return P.reshape(-1, 3), np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)], 0)


def flat(pkg):
    V, I = _grid((0, 0, 0), (8, 0, 0), (0, 0, 8), 16, 16)
    assert (V[:, 1] == 0).all()
    light = dict(position=(8.0, 0.0, 0.0), u=(0.0, 0.0, 0.25), v=(0.25, 0.0, 0.0), emission=(5, 5, 5))   # in the plane, beside the grid's corner, facing +y
    return _scene(pkg, "flat", V, I, light)


def _far_cornell(pkg, name, T):
    s = pkg.scenes.cornell_box()
    T = np.asarray(T, dtype=np.float64)
    V = (s.vertices.astype(np.float64) + T).astype(np.float32)
    L = dict(s.lights[0])
    L["position"] = tuple(float(x) for x in (np.asarray(L["position"], dtype=np.float32).astype(np.float64) + T).astype(np.float32))
    cam = dict(s.camera, eye=tuple(np.asarray(s.camera["eye"]) + T), lookat=tuple(np.asarray(s.camera["lookat"]) + T))
    return pkg.api.Scene(vertices=V, indices=s.indices, tri_material=s.tri_material, materials=s.materials, lights=[L], texcoords=s.texcoords,
                         camera=cam, name=name)


def far_tiles(pkg, name="far_tiles", edge=0.25, offset=FAR_64):
    """12 x 12 separate tiles (two triangles each, corners of their own) on the floor y = 0 and on the four walls; the light is the ceiling"""
    n = 12
    T = np.asarray(offset, dtype=np.float64)
    P = []
    for a, b, c, at in ((0, 2, 1, 0), (1, 2, 0, 0), (0, 1, 2, 0), (1, 2, 0, n), (0, 1, 2, n)):   # in-plane axes a, b; the plane: axis c = at x edge
        for i in range(n):
            for j in range(n):
                q = np.full((4, 3), at * edge)
                q[:, a] = np.array([i, i + 1, i + 1, i]) * edge
                q[:, b] = np.array([j, j, j + 1, j + 1]) * edge
                P.append(q[[0, 1, 2]]); P.append(q[[0, 2, 3]])
    P = (np.asarray(P) + T).astype(np.float32)
    V, I = _soup(P)
    w = n * edge
    pos = (np.array([0.0, w, 0.0]) + T).astype(np.float32)
    light = dict(position=tuple(float(x) for x in pos), u=(w, 0.0, 0.0), v=(0.0, 0.0, w), emission=(5, 5, 5))   # the ceiling; cross(u, v) = -y
    return _scene(pkg, name, V, I, light)


def _room(lo, hi):
    """the 12 triangles of the closed cube [lo, hi]^3"""
    room = []
    for axis in range(3):
        a, b = [k for k in range(3) if k != axis]
        for x in (lo, hi):
            q = np.full((4, 3), float(x))
            q[:, a] = (lo, hi, hi, lo)
            q[:, b] = (lo, lo, hi, hi)
            room += [q[[0, 1, 2]], q[[0, 2, 3]]]
    return np.asarray(room)


def duplicates(pkg):
    rng = _rng("duplicates")
    c = rng.uniform(0.5, 2.5, (64, 1, 3))
    base = (c + rng.uniform(-0.6, 0.6, (64, 3, 3))).astype(np.float32)
    P = [base] * 9
    # zero-area triangles on a dyadic grid (multiples of 1 / 64: every float64 cross product of their edges is exactly zero)
    p0 = np.round(rng.uniform(0.5, 2.5, (32, 3)) * 64) / 64
    e = np.round(rng.uniform(-0.5, 0.5, (32, 3)) * 64) / 64
    e[np.abs(e).sum(1) == 0] = 1 / 64
    p2 = np.round(rng.uniform(0.5, 2.5, (32, 3)) * 64) / 64
    Z = np.zeros((32, 3, 3))
    for i in range(32):
        Z[i] = ((p0[i], p0[i], p2[i]), (p0[i], p0[i] + e[i], p0[i] + 2 * e[i]), (p0[i], p0[i], p0[i]))[i % 3]
    P = np.concatenate(P + [Z.astype(np.float32)])
    P = np.concatenate([P[rng.permutation(len(P))], _room(-0.5, 3.5).astype(np.float32)])   # (a closed room: the rays that miss them hit something)
    V, I = _soup(P)
    light = dict(position=(1.0, 3.45, 1.0), u=(1.0, 0.0, 0.0), v=(0.0, 0.0, 1.0), emission=(5, 5, 5))   # under the ceiling, faces -y
    return _scene(pkg, "duplicates", V, I, light)


def _random_triangles(rng, centres, size):
    """triangles of about `size` (per triangle) around `centres`"""
    n = len(centres)
    size = np.broadcast_to(np.asarray(size, dtype=np.float64), (n,))
    return centres[:, None, :] + rng.uniform(-0.5, 0.5, (n, 3, 3)) * size[:, None, None]


def mixed_scale(pkg, name="mixed_scale", ground=40.0, small=(0.03, 0.1)):
    rng = _rng("mixed_scale")
    g = 0.5 * ground
    ground = np.array([[(-g, 0, -g), (-g, 0, g), (g, 0, g)], [(-g, 0, -g), (g, 0, g), (g, 0, -g)]], dtype=np.float64)   # faces +y
    small = _random_triangles(rng, rng.uniform(0.05, 0.95, (300, 3)), rng.uniform(small[0], small[1], 300))
    c = rng.uniform(-2.5, 3.5, (100, 3))
    c[:, 1] = rng.uniform(0.6, 2.5, 100)
    medium = _random_triangles(rng, c, 1.0)
    V, I = _soup(np.concatenate([ground, small, medium]))
    light = dict(position=(0.0, 3.5, 0.0), u=(1.0, 0.0, 0.0), v=(0.0, 0.0, 1.0), emission=(5, 5, 5))   # faces -y
    return _scene(pkg, name, V, I, light)


def nested(pkg, name="nested", factor=0.95):
    """triangle i has size 4 x factor^i and sits at that distance from the corner (0, 0, 0): every SAH cut peels the largest ones off.  A
    closed room of 12 triangles around them gives the rays that miss them something to hit."""
    rng = _rng("nested")
    s = 4.0 * factor ** np.arange(120)
    c = s[:, None] * np.array([1.0, 0.6, 0.8])[None, :]
    P = _random_triangles(rng, c, s)
    lo, hi = -2.5, 6.5
    V, I = _soup(np.concatenate([P, _room(lo, hi)]))
    light = dict(position=(0.0, hi - 0.05, 0.0), u=(3.0, 0.0, 0.0), v=(0.0, 0.0, 3.0), emission=(5, 5, 5))   # under the ceiling, faces -y
    return _scene(pkg, name, V, I, light)


def make(pkg, name, kw):
    if name.startswith("tiny_"):
        return tiny(pkg, **kw)
    if name in ("far_64", "far_256", "far_4096"):
        return _far_cornell(pkg, name, kw["offset"])
    for fn in (far_tiles, mixed_scale, nested):
        if name.startswith(fn.__name__):
            return fn(pkg, name=name, **kw)
    return globals()[name](pkg, **kw)


def ray_box(P):
    """the bounding box of the verdict's triangles (light corners included), grown about its centre to at least 1 unit per axis"""
    lo, hi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
    grow = np.maximum(0.0, 1.0 - (hi - lo)) * 0.5
    return lo - grow, hi + grow


_BUILT = {}


def build_scene_cases(pkg, name, kw, families=None):
    """ray_families.build_scene_cases for a hard scene: scene, verdict and, per family, the rays (from the grown box) with their float64 table;
    built once per scene and session, shared by every entry point and never written to."""
    if families is None:
        families = tuple(f for f in rf.FAMILIES if f not in NO_FAMILY.get(name, ()))
    key = (name, tuple(sorted(kw.items())), tuple(families))
    if key not in _BUILT:
        scene = make(pkg, name, kw)
        P, culled, ids = rv.scene_triangles(scene)
        V = rv.Verdict(P, culled)
        lo, hi = ray_box(P)
        cases = {}
        for f in families:
            fam = rf.family(f, name, P, lo, hi)
            fam["table"] = V.table(fam["rays"], fam["tmax_any"])
            cases[f] = fam
        _BUILT[key] = dict(scene=scene, verdict=V, ids=ids, cases=cases, name=name, box=(lo, hi))
    return _BUILT[key]


# ---- the built tree, without a GPU: tests/native/lbvh_check.cpp on the verdict's triangles (the order spcbpt_create hands the builder) ------
def write_mesh(path, P):
    """the mesh format of tools/bvh_eval.cpp: int32 nv, nt; float32 vertices[nv][3]; uint32 indices[nt][3]"""
    P = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 3)
    with open(path, "wb") as f:
        f.write(np.array([len(P), len(P) // 3], np.int32).tobytes())
        f.write(P.tobytes())
        f.write(np.arange(len(P), dtype=np.uint32).tobytes())


_CHECKER = {}


def checker(sanitize=False):
    """tests/native/lbvh_check.cpp as a stand-alone program (with the sanitizers for the structural test, plain for tree_info)"""
    if sanitize not in _CHECKER:
        d = tempfile.mkdtemp(prefix="lbvh_check_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        exe = os.path.join(d, "lbvh_check")
        flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
        subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags + ["-o", exe, os.path.join(ROOT, "tests", "native", "lbvh_check.cpp")], check=True)
        _CHECKER[sanitize] = exe
    return _CHECKER[sanitize]


def tree_info(P, builder="sah"):
    """dict(n, nodes, depth, root_slots, ...) of the tree build_lbvh makes of triangles P: the last line of the checker's output"""
    with tempfile.TemporaryDirectory() as d:
        mesh = os.path.join(d, "mesh.bin")
        write_mesh(mesh, P)
        r = subprocess.run([checker(), "mesh", mesh], env=dict(os.environ, SPCBPT_BVH=builder), capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
    return {k: float(v) if "." in v else int(v) for k, v in re.findall(r"(\w+)=([-+.\de]+)", r.stdout.strip().splitlines()[-1])}
