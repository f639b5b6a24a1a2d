"""Record families for the eye-side definition (tests/connect_ref.py), shared by tests/test_connect_definition_cpu.py and
tests/test_gpu_connect_definition.py (a helper, not a test).

A world is one of the project's smallest scenes with two materials appended that no triangle carries (the 0.0005-roughness metal
below the alpha clamp and an all-lobes Disney material: records name them by id), the oracle on it, and a subspace tuple made for
this audit: the trees of parity_util.grid_tree_tuple (one octree level and a normal split, no direction nodes; eye labels 101 ..
121, light labels 301 .. 321: disjoint, a transposed index reads another cell), every eye row a seeded random CMF of its own, Q
drawn at random with a handful of zero-handled cells (Q = FLT_MAX and no mass in any row, as Q_zero_handle leaves an empty subspace:
Gamma^ is exactly 0 there).  The tuple is not unbiased; nothing is rendered.

Every record keeps its indices in range: labels and zones in [0, NUM_SUBSPACE), material ids that exist, finite positions.  Cached
label words outside the label range are NOT fed to anything: a broken guard would read past the Gamma table, and this suite does not
go looking for faults."""
import numpy as np

from tests import connect_ref as R
from tests.parity_util import cornell_with_flagged_box, grid_trees

EYE_LABELS = np.array([102, 103, 104, 105, 106, 107, 108, 120, 121])
LIGHT_LABELS = np.array([302, 303, 304, 305, 306, 307, 308, 320, 321])
ZERO_CELLS = np.array([320, 103, 640])               # zero-handled: a light-tree leaf, an eye-tree leaf, an unused cell
ZERO_LIGHT = 320
SHARP = dict(color=(0.9, 0.85, 0.6), roughness=0.0005, metallic=1.0)
ALL_LOBES = dict(color=(0.55, 0.3, 0.7), roughness=0.35, metallic=0.3, specular=0.8, specular_tint=0.4, subsurface=0.3, sheen=0.6,
                 sheen_tint=0.7, clearcoat=0.8, clearcoat_gloss=0.6)
FLAGS = np.uint32(R.LV_DIRECTION | R.LV_LAST_DIRECTION)
N_CAMERA = 3072


def scene_of(pkg, which):
    scene = dict(cornell=pkg.scenes.cornell_box, flagged=lambda: cornell_with_flagged_box(pkg, roughness=0.3), courtyard=pkg.scenes.courtyard)[which]()
    scene.materials = list(scene.materials) + [dict(SHARP), dict(ALL_LOBES)]
    return scene


def legal_forms(which):
    """cornell is plain (DeviceScene::general == 0); a flagged material and the sky make the other two general"""
    return R.FORMS if which == "cornell" else R.FORMS[:2]


def audit_tuple(pkg, scene, seed=17):
    et, lt = grid_trees(pkg, scene)
    rng = np.random.default_rng(seed)
    n = pkg.NUM_SUBSPACE
    mass = rng.uniform(0.05, 1.0, (n, n))
    mass[:, ZERO_CELLS] = 0.0
    cmf = np.cumsum(mass, 1)
    cmf = np.maximum.accumulate((cmf / cmf[:, -1:]).astype(np.float32), 1)
    cmf[:, -1] = 1.0
    q = rng.uniform(0.2, 2.0, n).astype(np.float32)
    q[ZERO_CELLS] = np.float32(R.FLT_MAX)
    return et, lt, q, cmf


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def camera_records(pkg, ob, scene, n, rng, aspect):
    cam = scene.camera
    U, V, Wv = pkg.camera_frame(np.array(cam["eye"], np.float32), np.array(cam["lookat"], np.float32), np.array(cam["up"], np.float32),
                                np.float32(cam["fov"]), np.float32(aspect))
    d = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    dirs = f32(_unit(d[:, :1] * U[None, :] + d[:, 1:] * V[None, :] + Wv[None, :]))
    rec = np.zeros(n, ob.EYE_STEP_IN_DTYPE)
    rec["last"]["position"] = cam["eye"]; rec["last"]["normal"] = dirs; rec["last"]["flux"] = 1.0
    rec["last"]["last_position"] = cam["eye"]; rec["last"]["pdf"] = 1.0; rec["last"]["single_pdf"] = 1.0
    rec["next_single_pdf"] = 1.0
    rec["seed"] = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    rec["dir"] = dirs
    return rec


def build_world(pkg, ob, which, seed=1):
    """The oracle on scene `which` with the audit's tuple, its light-vertex cache, and four levels of its own eye walk: `steps` =
    the EYE_STEP input records of every level, `eye` = the surface vertices they produced (depth 1 .. 4)."""
    scene = scene_of(pkg, which)
    W, H = 64, 36
    o = ob.Oracle(scene)
    cam = scene.camera
    o.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
    o.resize(W, H)
    env = scene.environment
    if env is not None:
        o.set_environment(env["rgba"], env["center"], env["radius"])
    o.set_light_trace(1500, 64, 1)
    tup = audit_tuple(pkg, scene)
    o.set_subspace(*tup)
    o.launch("light trace", 11)
    lvc = o.lvc_read()
    rng = np.random.default_rng(seed)
    rec = camera_records(pkg, ob, scene, N_CAMERA, rng, W / H)
    steps, eye = [], []
    for level in range(1, 5):
        out = o.eye_step(rec)
        steps.append(rec)
        eye.append(out["mid"][out["kind"] == 1].copy())
        go = (out["kind"] == 1) & (out["done"] == 0)
        nxt = np.zeros(int(go.sum()), ob.EYE_STEP_IN_DTYPE)
        nxt["last"] = out["mid"][go]; nxt["next_flux"] = out["next_flux"][go]; nxt["next_single_pdf"] = out["next_single_pdf"][go]
        nxt["seed"] = out["seed"][go]; nxt["dir"] = out["dir"][go]
        rec = nxt
    lights = R.scene_lights(scene, env)
    return dict(which=which, scene=scene, o=o, tup=tup, lvc=lvc, env=env, steps=np.concatenate(steps), eye=np.concatenate(eye), W=W, H=H,
                n_mat=len(scene.materials), project_pdf=1.0 / (np.pi * lights[-1]["r"] ** 2) if env is not None else 0.0,
                extent=float(np.linalg.norm(scene.vertices.max(0) - scene.vertices.min(0))))


# ---- labels as the device passes store them -----------------------------------------------------------------------------------------
def own_lsub(w, a):
    """an eye vertex's own light-tree label as eye_surface_hit caches it (0 at depth 1, where nothing reads it)"""
    return np.where(a["depth"] >= 2, R.tree_labels(w["tup"][1], a["position"], a["normal"]), 0)


def with_own_pad(w, b):
    """pad = the flag bits | (own eye-tree label + 1) on a surface vertex, as the light pass fills it; an origin keeps label word 0"""
    b = b.copy()
    lab = R.tree_labels(w["tup"][0], b["position"], b["normal"]) + 1
    b["pad"] = (b["pad"] & FLAGS) | np.where(b["depth"] > 0, lab, 0).astype(np.uint32)
    return b


def _other(labels, own, rng):
    """for every record a label of `labels` that differs from its own"""
    pick = labels[rng.integers(0, len(labels), len(own))]
    return np.where(pick == own, labels[(np.searchsorted(labels, pick) + 1) % len(labels)], pick)


def _perp(v, rng):
    t = np.cross(v, _unit(rng.normal(size=v.shape)))
    return _unit(t)


def _pairs(w, rng, n, origins=0.3, sel_b=None):
    ev, lvc = w["eye"], w["lvc"]
    a = ev[rng.integers(0, len(ev), n)].copy()
    org = np.nonzero(lvc["depth"] == 0)[0]
    pick = np.where(rng.uniform(0, 1, n) < origins, rng.choice(org, n), rng.integers(0, len(lvc), n))
    if sel_b is not None:
        pick = rng.choice(np.nonzero(sel_b)[0], n)
    return a, with_own_pad(w, lvc[pick])


def connect_families(w, seed=3, n=3000):
    """{family: dict(a, b, lsub, forms, judge_value (None: every record), tree_labels: the records carry the trees' own labels)}"""
    rng = np.random.default_rng(seed)
    forms, cached = legal_forms(w["which"]), tuple(f for f in legal_forms(w["which"]) if f != "reference")
    F = {}

    def add(name, a, b, lsub=None, forms=forms, judge_value=None, tree=True):
        keep = np.ones(len(a), bool)
        if name != "grazing":
            # two vertices on the same face that is not axis-aligned are coplanar to rounding, not exactly: cosines of 1e-8 of which no
            # digit is computable.  The families leave such pairs out (the grazing family sets its cosines itself), so that the
            # ill-conditioned share stays a statement about the arithmetic
            c = _unit(a["position"].astype(np.float64) - b["position"].astype(np.float64))
            sa, sb = np.abs((a["normal"] * -c).sum(1)), np.abs((b["normal"] * c).sum(1))
            sb = np.where((b["pad"] & np.uint32(R.LV_DIRECTION)) != 0, 1.0, sb)
            keep = ((sa == 0) | (sa > 1e-4)) & ((sb == 0) | (sb > 1e-4))
            a, b, lsub = a[keep], b[keep], None if lsub is None else lsub[keep]
        F[name] = dict(a=a, b=b, lsub=own_lsub(w, a) if lsub is None else lsub, forms=forms, judge_value=judge_value, tree_labels=tree)
        return keep

    # real eye vertices of depth 1 .. 4 x real light vertices (a third of them origins)
    a, b = _pairs(w, rng, n)
    add("chain", a, b)
    # the stored labels differ from the trees': the stored ones must be used (an origin's label word is never read)
    b2 = b.copy()
    own_e = (b["pad"] & np.uint32(0xffff)).astype(np.int64) - 1
    b2["pad"] = (b["pad"] & FLAGS) | (_other(EYE_LABELS, own_e, rng) + 1).astype(np.uint32)
    add("stored labels differ from the trees'", a, b2, lsub=_other(LIGHT_LABELS, own_lsub(w, a), rng), forms=cached, tree=False)
    # label word 0 (an imported cache): the descent must happen on a surface vertex; an emitter vertex needs none
    b3 = b.copy()
    b3["pad"] = b["pad"] & FLAGS
    add("label word 0", a, b3, forms=cached)
    # b.depth == 0 seen from the front and from behind
    a, b = _pairs(w, rng, n, sel_b=(w["lvc"]["depth"] == 0) & ((w["lvc"]["pad"] & np.uint32(R.LV_DIRECTION)) == 0))
    flip = rng.uniform(0, 1, n) < 0.5
    b["normal"] = np.where(flip[:, None], -b["normal"], b["normal"])
    add("emitter vertex from the front and from behind", a, b)
    # grazing pairs: a.n . d and b.n . d in {+-1e-3, +-1e-6, exactly 0}
    a, b = _pairs(w, rng, n, origins=0.5, sel_b=(w["lvc"]["pad"] & np.uint32(R.LV_DIRECTION)) == 0)
    vals = np.array([1e-3, -1e-3, 1e-6, -1e-6, 0.0])
    sa, sb = vals[rng.integers(0, 5, n)], vals[rng.integers(0, 5, n)]
    zero = (sa == 0) | (sb == 0)
    b["position"][zero, 1] = a["position"][zero, 1]            # c.y == 0 exactly: an axis-aligned normal gives an exact zero
    c = _unit(a["position"].astype(np.float64) - b["position"].astype(np.float64))
    na = sa[:, None] * -c + np.sqrt(1 - sa**2)[:, None] * _perp(c, rng)
    nb = sb[:, None] * c + np.sqrt(1 - sb**2)[:, None] * _perp(c, rng)
    up = np.array([0.0, 1.0, 0.0])
    na, nb = np.where((sa == 0)[:, None], up * rng.choice([-1.0, 1.0], (n, 1)), na), np.where((sb == 0)[:, None], up * rng.choice([-1.0, 1.0], (n, 1)), nb)
    a["normal"], b["normal"] = f32(na), f32(nb)
    a["last_position"] = f32(a["position"] + 0.4 * na + 0.2 * _perp(na, rng))    # the predecessors above the surfaces
    b["last_position"] = f32(b["position"] + 0.4 * nb + 0.2 * _perp(nb, rng))
    # at |n . d| = 1e-6 one ulp of the direction moves the cosine, and with it value and weight, by a tenth: those records carry the
    # sign and zero checks only (every record does); value and weight are judged where both cosines are +-1e-3
    add("grazing", a, with_own_pad(w, b), judge_value=(np.abs(sa) == 1e-3) & (np.abs(sb) == 1e-3))
    F["grazing"].update(sa=sa, sb=sb)
    # short connections: |a.P - b.P| from SCENE_EPSILON upwards; the value crosses the 1e5 of ISINVALIDVALUE
    a, b = _pairs(w, rng, n, origins=0.0, sel_b=(w["lvc"]["depth"] > 0) & ((w["lvc"]["pad"] & FLAGS) == 0))
    na = a["normal"].astype(np.float64)
    d = _unit(na + 0.6 * _perp(na, rng))
    ell = R.SCENE_EPSILON * 10.0 ** rng.uniform(0.0, 2.5, n)
    b["position"] = f32(a["position"] + ell[:, None] * d)
    nb = _unit(-d + 0.5 * _perp(d, rng))
    b["normal"] = f32(nb)
    b["last_position"] = f32(b["position"] + 0.5 * nb + 0.3 * _perp(nb, rng))
    # (the weight falls as the geometry term rises, so the value stays of order 1 however short the segment: a bright eye
    # sub-path carries it across the threshold)
    a["flux"] = f32(a["flux"] * 10.0 ** rng.uniform(4.0, 7.0, (n, 1)))
    add("short connections", a, with_own_pad(w, b))
    # zero-handled Q cells on every lookup; 0 / 0 where nothing else carries weight (a.depth == 1, b without a recursion term)
    a, b = _pairs(w, rng, n)
    k = rng.integers(0, 4, n)
    b["subspace_id"] = np.where(k == 0, ZERO_LIGHT, b["subspace_id"])
    b["last_zone_id"] = np.where((k == 1) | (k == 3), ZERO_LIGHT, b["last_zone_id"])
    lsub = np.where(k == 2, ZERO_LIGHT, own_lsub(w, a))
    z = (k == 3) & (a["depth"] == 1) & (b["depth"] > 0)
    b["subspace_id"] = np.where(z, ZERO_LIGHT, b["subspace_id"])
    b["rmis_pointer"] = np.where(z, 0.0, b["rmis_pointer"]).astype(np.float32)
    keep = add("zero-handled Q cells", a, b, lsub=lsub, tree=False)
    F["zero-handled Q cells"]["zero_over_zero"] = z[keep]
    # the alpha-clamped metal and the all-lobes material on either vertex
    a, b = _pairs(w, rng, n)
    k = rng.integers(0, 8, n)            # the narrow lobe on an eighth of the eye and of the light vertices: its poles stay inside ILL_CAP
    a["material_id"] = np.where(k == 0, w["n_mat"] - 2, np.where((k == 1) | (k == 4), w["n_mat"] - 1, a["material_id"]))
    surf = b["depth"] > 0
    b["material_id"] = np.where(surf & (k == 2), w["n_mat"] - 2, np.where(surf & ((k == 3) | (k == 5)), w["n_mat"] - 1, b["material_id"]))
    a["color"] = np.where(np.isin(k, (0, 1, 4))[:, None], f32(rng.uniform(0.05, 1.0, (n, 3))), a["color"])
    add("alpha-clamped and all-lobes materials", a, b)
    if w["env"] is not None:
        pad = w["lvc"]["pad"]
        a, b = _pairs(w, rng, n, sel_b=(pad & np.uint32(R.LV_DIRECTION)) != 0)
        add("sky directions", a, b)
        a, b = _pairs(w, rng, n, sel_b=(pad & np.uint32(R.LV_LAST_DIRECTION)) != 0)
        add("light vertices lit straight by the sky", a, b)
    for name, f in F.items():
        check_ranges(w, f["a"], f["b"], f["lsub"], name)
    return F


def check_ranges(w, a, b, lsub, name):
    n = R.NUM_SUBSPACE
    for x in (a["subspace_id"], a["last_zone_id"], b["subspace_id"], b["last_zone_id"], lsub):
        assert ((np.asarray(x) >= 0) & (np.asarray(x) < n)).all(), name
    lab = (b["pad"] & np.uint32(0xffff)).astype(np.int64)
    assert (lab <= n).all(), name                                   # 0 (none) or a label + 1: nothing beyond the table is ever fed
    assert ((a["material_id"] >= 0) & (a["material_id"] < w["n_mat"])).all() and ((b["material_id"] >= 0) & (b["material_id"] < w["n_mat"]))[b["depth"] > 0].all(), name
    for x in (a["position"], a["last_position"], b["position"], b["last_position"], a["normal"], b["normal"]):
        assert np.isfinite(x).all(), name


def eye_step_families(w, seed=5):
    """{family: dict(rec (EYE_STEP_IN_DTYPE), lsub, forms)}: the four levels of the oracle's walk in one array"""
    rng = np.random.default_rng(seed)
    forms, cached = legal_forms(w["which"]), tuple(f for f in legal_forms(w["which"]) if f != "reference")
    rec = w["steps"]
    own = own_lsub(w, rec["last"])
    F = {"walk": dict(rec=rec, lsub=own, forms=forms, tree_labels=True)}
    # (the whole walk again: the word is read behind depth 2 only, and the family's ill-conditioned share stays the walk's)
    F["stored lsub differs from the tree's"] = dict(rec=rec, lsub=_other(LIGHT_LABELS, own, rng), forms=cached, tree_labels=False)
    F["zero-handled cell in lsub"] = dict(rec=rec, lsub=np.full(len(rec), ZERO_LIGHT), forms=cached, tree_labels=False)
    r2 = rec[rec["last"]["depth"] >= 1].copy()
    k = rng.integers(0, 4, len(r2))
    r2["last"]["material_id"] = np.where(k == 0, w["n_mat"] - 2, w["n_mat"] - 1)
    r2["last"]["color"] = f32(rng.uniform(0.05, 1.0, (len(r2), 3)))
    F["alpha-clamped and all-lobes materials"] = dict(rec=r2, lsub=own_lsub(w, r2["last"]), forms=forms, tree_labels=True)
    for name, f in F.items():
        L = f["rec"]["last"]
        assert ((L["subspace_id"] >= 0) & (L["subspace_id"] < R.NUM_SUBSPACE) & (L["last_zone_id"] >= 0) & (L["last_zone_id"] < R.NUM_SUBSPACE)).all(), name
        assert ((f["lsub"] >= 0) & (f["lsub"] < R.NUM_SUBSPACE)).all() and ((L["material_id"] >= 0) & (L["material_id"] < w["n_mat"]))[L["depth"] > 0].all(), name
    return F


def clear_of_sky_borders(w, dirs, margin=1e-3):
    """within a thousandth of a texel of the map or of a cell of the sky's labels FP32 (u, v) may read the neighbour: the families leave
    such directions out, so that the audit's own count of them (LABEL_CAP, at 1e-4) stays a statement about rounding"""
    from tests import env_ref
    lights = R.scene_lights(w["scene"], w["env"])
    d64 = np.asarray(dirs, np.float64)
    return (env_ref.env_pdf(lights[-1]["raster"], d64)[1] >= margin) & (env_ref.env_label(d64, lights[-1]["div"])[1] >= margin)


def sky_miss_family(w, seed=7, n=3000):
    """escaped eye paths of depth 0 .. 4: (last vertex, NextVertex.flux, NextVertex.singlePdf, direction above the vertex's surface, lsub)"""
    rng = np.random.default_rng(seed)
    ev = w["eye"]
    last = ev[rng.integers(0, len(ev), n)].copy()
    nl = last["normal"].astype(np.float64)
    dirs = f32(_unit(nl * rng.uniform(0.05, 1.0, (n, 1)) + _perp(nl, rng) * rng.uniform(0.0, 1.0, (n, 1))))
    cam = w["steps"][w["steps"]["last"]["depth"] == 0][: n // 6]
    last[: len(cam)] = cam["last"]
    dirs[: len(cam)] = cam["dir"]
    up = rng.uniform(0, 1, n) < 0.7                         # most towards the upper sky, where the map is bright
    dirs[:, 1] = np.where(up & (last["depth"] > 0) & (nl[:, 1] >= 0), np.abs(dirs[:, 1]), dirs[:, 1])
    keep = clear_of_sky_borders(w, dirs)
    last, dirs = last[keep], dirs[keep]
    n = len(last)
    return dict(last=last, next_flux=f32(rng.uniform(0.05, 1.0, (n, 3))), next_single_pdf=f32(rng.uniform(0.1, 2.0, n)), dirs=dirs,
                lsub=own_lsub(w, last))
