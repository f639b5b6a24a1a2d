"""The float64 light-vertex-cache audit (tests/lvc_audit.py) on the CPU: the check of the check.

1. The ORACLE's cache passes the audit on the Cornell box (two launch geometries), the textured bedroom and the courtyard with its
   environment map: the audit's definitions are the reference's.  Every run prints the error quantiles the bars of lvc_audit.BARS
   were derived from (run with -s).
2. The audit sees what it is for: one seeded corruption at a time, applied to about 0.3 % of the records of a passing cache, makes
   exactly its own check fail; the message names the scenario, the count and records that were corrupted, and the failure lists at
   least 90 % of the corrupted records and no other.  A corruption is applied
   to records that END their path (no later record reads them), so that "its own check" is well defined; where one wrong quantity
   enters two stored fields (pdf_G enters single_pdf and flux; a stored single_pdf that no longer multiplies to the stored pdf) the
   expected set names both."""
import numpy as np
import pytest

from tests import lvc_audit as A
from tests.parity_util import minimal_tuple

SCENARIOS = {
    "cornell (3000, 64, 2)": ("cornell", (3000, 64, 2)),
    "cornell (60, 48, 40)": ("cornell", (60, 48, 40)),
    "bedroom (2000, 64, 1)": ("bedroom", (2000, 64, 1)),
    "courtyard, sky (8000, 64, 1)": ("courtyard", (8000, 64, 1)),
}


def oracle_cache(pkg, ob, which, lt, frame=7):
    scene = dict(cornell=pkg.scenes.cornell_box, courtyard=pkg.scenes.courtyard,
                 bedroom=lambda: pkg.scenes.bedroom(target_tris=8000, tex_size=64))[which]()
    o = ob.Oracle(scene)
    cam = scene.camera
    o.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], 1.0)
    o.resize(8, 8)
    env = scene.environment
    if env is not None:
        o.set_environment(env["rgba"], env["center"], env["radius"])
    o.set_light_trace(*lt)
    tup = minimal_tuple(o, 2)
    o.set_subspace(*tup)
    o.launch("light trace", frame)
    lvc = o.lvc_read()
    o.build_sampler()
    return dict(scene=scene, tup=tup, lvc=lvc, lt=lt, env=env, paths=o.sampler_read()[4])


def run_audit(w, lvc=None, name="oracle", report=print):
    lvc = w["lvc"] if lvc is None else lvc
    res = A.audit(w["scene"], w["tup"], lvc, w["lt"], env=w["env"], path_count=w["paths"])
    return res, A.judge(res, lvc, name, report=report)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_the_oracles_cache_passes_the_audit(pkg, ob, name):
    w = oracle_cache(pkg, ob, *SCENARIOS[name])
    res, fails = run_audit(w, name="oracle, " + name)
    assert not fails, "\n".join(m for _, m in fails)
    assert len(w["lvc"]) > 2500
    n_step = len(res["last_lum"].err)
    assert n_step + len(res["origin: position"].err) == len(w["lvc"])          # every record judged: origins + steps = the cache
    assert len(res["single_pdf"].err) + len(res["single_pdf depth 1"].err) == n_step
    if w["env"] is not None:
        lld = (w["lvc"]["pad"] & A.LV_LAST_DIRECTION) != 0               # most sky paths miss the yard; those that land feed the `lld` branch
        st = res["_step"]
        assert len(res["origin pdf (sky)"].err) > 500 and lld.sum() > 100 and (lld[st["li"]] & st["deep"]).sum() > 50
    if SCENARIOS[name][1][2] > 1:      # cores that end because their slot range is full, in the middle of a path and right after an origin
        core = w["lvc"]["path_id"] // w["lt"][2]
        full = np.bincount(core, minlength=w["lt"][0]) == w["lt"][1]
        last = np.concatenate([core[1:] != core[:-1], [True]])
        if w["lt"][1] == 48:
            assert full.sum() > 10 and (w["lvc"]["depth"][last & full[core]] == 0).any() and (w["lvc"]["depth"][last & full[core]] > 0).any()


# ---------------------------------------------------------------------------------------------------------------- corruptions
@pytest.fixture(scope="module")
def cornell(pkg, ob):
    w = oracle_cache(pkg, ob, "cornell", (3000, 64, 2))
    res, fails = run_audit(w, report=lambda s: None)
    assert not fails
    w["res"] = res
    return w


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def _targets(w, rng, deep, extra=None):
    """About 0.3 % of the cache: rows (into the audit's step arrays) of records that end their path, at depth >= 2 or depth 1."""
    st, lvc = w["res"]["_step"], w["lvc"]
    mi = st["mi"]
    terminal = np.concatenate([lvc["path_id"][1:] != lvc["path_id"][:-1], [True]])[mi]
    ok = terminal & (st["deep"] if deep else ~st["deep"])
    if extra is not None:
        ok &= extra
    rows = np.nonzero(ok)[0]
    k = int(round(0.003 * len(lvc)))
    assert len(rows) >= k
    return np.sort(rng.choice(rows, k, replace=False))


def _no_rr(w, lvc, rows, st):
    i, l = st["mi"][rows], st["li"][rows]
    lvc["single_pdf"][i] = _f32(lvc["single_pdf"][i] / A.rr_of(lvc["color"][l]))
    lvc["pdf"][i] = lvc["pdf"][l] * lvc["single_pdf"][i]


def _stale_flux(w, lvc, rows, st):
    """next_flux left over in the lane's register from the path the same core walked before (its last surface vertex)"""
    i, l = st["mi"][rows], st["li"][rows]
    pid = lvc["path_id"][st["mi"]]
    for r, ii, ll in zip(rows, i, l):
        stale = st["base"]["next_flux"][np.nonzero(st["deep"] & (pid == lvc["path_id"][ii] - 1))[0][-1]]
        lvc["flux"][ii] = _f32(stale * lvc["flux"][ll].astype(np.float64) * st["base"]["pdf_g"][r])


def _no_inverse_square(w, lvc, rows, st):
    i, l = st["mi"][rows], st["li"][rows]
    t2 = st["base"]["t"][rows] ** 2
    lvc["single_pdf"][i] = _f32(lvc["single_pdf"][i] * t2)
    lvc["flux"][i] = _f32(lvc["flux"][i] * t2[:, None])
    lvc["pdf"][i] = lvc["pdf"][l] * lvc["single_pdf"][i]


def _last_lum_of_l(w, lvc, rows, st):
    lvc["last_lum"][st["mi"][rows]] = lvc["last_lum"][st["li"][rows]]


def _zone_off_by_one(w, lvc, rows, st):
    lvc["last_zone_id"][st["mi"][rows]] = lvc["subspace_id"][st["pi"][rows]]


def _ll_pdf_at_minus_d(w, lvc, rows, st):
    S = dict(st["S"], ll_sign=-np.ones(len(st["mi"])))
    zero = np.zeros((len(st["mi"]), 3))
    lvc["rmis_pointer"][st["mi"][rows]] = _f32(A._predict(S, zero, zero, zero)["rmis"][rows])


def _last_position_of_origin(w, lvc, rows, st):
    i = st["mi"][rows]
    lvc["last_position"][i] = lvc["position"][i - lvc["depth"][i]]


def _behind_the_box(w, lvc, rows, st):
    """A depth-1 vertex moved onto the floor UNDER the short box (the box has no bottom face: the floor there is a real surface of
    the scene, of the right material and normal, that no light path can reach), every field rebuilt consistently from the audit's own
    formulas: the vertex is a perfectly formed record of a walk that went through the top of the box."""
    i = st["mi"][rows]
    rng = np.random.default_rng(5)
    lvc["position"][i] = np.stack([0.4 + rng.uniform(-0.05, 0.05, len(i)), np.zeros(len(i)), 0.2 + rng.uniform(-0.05, 0.05, len(i))], 1).astype(np.float32)
    lvc["normal"][i] = (0.0, 1.0, 0.0)
    lvc["material_id"][i] = 0
    lvc["color"][i] = np.asarray(w["scene"].materials[0]["color"], np.float32)
    res = A.audit(w["scene"], w["tup"], lvc, w["lt"])
    s2 = res["_step"]
    rows2 = np.searchsorted(s2["mi"], i)
    lvc["single_pdf"][i] = _f32(s2["base"]["single_pdf"][rows2])
    lvc["flux"][i] = _f32(s2["base"]["flux"][rows2])
    lvc["last_normal_projection"][i] = _f32(s2["base"]["lnp"][rows2])
    lvc["pdf"][i] = lvc["pdf"][i - 1] * lvc["single_pdf"][i]


def _swap(w, lvc, rows, st):
    i = st["mi"][rows]                   # rows: depth-2 records; swapped with their depth-1 predecessor
    a, b = lvc[i].copy(), lvc[i - 1].copy()
    lvc[i], lvc[i - 1] = b, a


CORRUPTIONS = {
    # name: (deep?, corruption, the checks that must fail -- and no other)
    "next_single_pdf without the rr factor": (True, _no_rr, {"single_pdf"}),
    "flux from the next_flux of the core's previous path": (True, _stale_flux, {"flux"}),
    "pdf_G without 1 / t^2": (True, _no_inverse_square, {"single_pdf", "flux"}),
    "last_lum taken from l.last_lum": (True, _last_lum_of_l, {"last_lum"}),
    "last_zone_id off by one vertex": (True, _zone_off_by_one, {"last_zone_id"}),
    "rmis_pointer with LL_pdf evaluated at -d": (True, _ll_pdf_at_minus_d, {"rmis_pointer"}),
    "last_position left at the origin's": (True, _last_position_of_origin, {"last_position"}),
    "a depth-1 vertex moved behind a wall of the box": (False, _behind_the_box, {"segment is clear"}),
    "two records of a path swapped": (True, _swap, {"structure: predecessor"}),
}


def _changed(before, after, idx):
    """the records of idx a corruption really changed (a zero flux times 1.001, the last_lum of a path that carries no light: no change)"""
    return np.array([i for i in idx if before[i].tobytes() != after[i].tobytes()], np.int64)


def _check_messages(fails, lvc_before, idx, scenario, cover=(), core=None, share=0.9):
    """Every message names the scenario, its check, a count and records that were corrupted; the failures of the checks in `cover`
    name (Failure.records) at least `share` of the corrupted records `core`, and nothing but corrupted records."""
    hit = {(int(lvc_before["path_id"][i]), int(lvc_before["depth"][i])) for i in idx}
    core = idx if core is None else core
    for f in fails:
        name, msg = f
        assert np.isin(f.records, idx).all(), (name, f.records[~np.isin(f.records, idx)][:5])
        if name in cover:
            assert len(core) >= 30 and np.isin(core, f.records).mean() >= share, (name, float(np.isin(core, f.records).mean()), msg)
        assert msg.startswith(f"{scenario}: {name}: "), msg
        count = int(msg.split(": ")[2 + name.count(": ")].split(" of ")[0])
        assert 1 <= count, msg
        named = [tuple(int(x) for x in s.strip("()").split(", ")) for s in msg.split("first: ")[1].replace("), (", ")|(").split("|")]
        assert named and all(p in hit for p in named), (msg, sorted(hit)[:5])
    return True


@pytest.mark.parametrize("what", list(CORRUPTIONS))
def test_a_corruption_fails_exactly_its_own_check(cornell, what):
    deep, corrupt, expected = CORRUPTIONS[what]
    w, st = cornell, cornell["res"]["_step"]
    rng = np.random.default_rng(sum(map(ord, what)))
    extra = None
    if corrupt is _no_inverse_square:
        extra = np.abs(st["base"]["t"] ** 2 - 1.0) > 0.05
    if corrupt is _zone_off_by_one:
        extra = w["lvc"]["subspace_id"][st["pi"]] != w["lvc"]["subspace_id"][st["li"]]
    if corrupt is _stale_flux:
        pid = w["lvc"]["path_id"][st["mi"]]                      # the second path of a core whose first path has a surface vertex behind depth 1
        extra = (pid % w["lt"][2] == 1) & np.isin(pid - 1, pid[st["deep"]])
    if corrupt is _swap:
        extra = w["lvc"]["depth"][st["mi"]] == 2
    rows = _targets(w, rng, deep, extra)
    lvc = w["lvc"].copy()
    corrupt(w, lvc, rows, st)
    idx = core = st["mi"][rows]
    if corrupt is _swap:
        core = np.concatenate([idx - 1, idx])                # both records of the pair sit behind the wrong predecessor ...
        idx = np.concatenate([core, idx + 1])                # ... and so does the record behind them, if the path goes on
    res, fails = run_audit(w, lvc, name=what, report=lambda s: None)
    assert A.failed_checks(fails) == sorted(expected), [m for _, m in fails]
    _check_messages(fails, lvc, idx, what, cover=expected, core=_changed(w["lvc"], lvc, core))


# the check a relative perturbation of 1e-3 of one float field of a record must trip -- `only`: and no other check
FIELD_CHECK = {
    "position": ("position on a triangle of the material", False),     # the moved point also changes d and t: the measures fail with it
    "normal": ("normal", False),                                       # ... and |m.n . d|
    "pdf": ("pdf", True),
    "single_pdf": ("single_pdf", False),                               # ... and pdf: the stored pdf is no longer l.pdf x the stored single_pdf
    "flux": ("flux", True),
    "rmis_pointer": ("rmis_pointer", True),
    "color": ("color", True),
    "last_lum": ("last_lum", True),
    "last_position": ("last_position", True),
    "last_normal_projection": ("last_normal_projection", True),
}


@pytest.mark.parametrize("field", A.FLOAT_FIELDS)
def test_a_relative_perturbation_of_1e_3_is_seen(cornell, field):
    w, st = cornell, cornell["res"]["_step"]
    # (the projection is judged absolutely, a cosine: 1e-3 of it shows where the cosine itself is not small)
    rows = _targets(w, np.random.default_rng(A.FLOAT_FIELDS.index(field)), True, extra=st["base"]["lnp"] > 0.05 if field == "last_normal_projection" else None)
    lvc = w["lvc"].copy()
    idx = st["mi"][rows]
    lvc[field][idx] = lvc[field][idx] * np.float32(1.001)
    res, fails = run_audit(w, lvc, name=field, report=lambda s: None)
    own, only = FIELD_CHECK[field]
    failed = A.failed_checks(fails)
    assert own in failed and (not only or failed == [own]), [m for _, m in fails]
    if field == "single_pdf":
        assert failed == ["pdf", "single_pdf"]
    # (a point moved WITHIN its triangle's plane -- a coordinate that is 0, an axis-aligned wall -- still lies on it: the measures name it)
    _check_messages(fails, lvc, idx, field, cover=[own], core=_changed(w["lvc"], lvc, idx), share=0.8 if field == "position" else 0.9)
