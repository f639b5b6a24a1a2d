"""The eye side of the estimator on the device, held to its float64 definition (tests/connect_ref.py) record by record, in every
form the timed kernels run.

spcbpt_debug_unit's CONNECT / EYE_STEP / SKY_MISS take a form word (include/spcbpt.h): `reference` (CACHE = false, ENV = true: labels by
descent), `cached` (CACHE = true, ENV = true: the timed kernels of a general scene) and `cached_plain` (CACHE = true, ENV = false: the
timed kernels of the Cornell box and the bench scene).  Every record family of tests/connect_families.py runs through every form
that is legal for its scene, one launch per family and form, and is judged by the audit at the bars connect_ref.BARS derives from
the ORACLE's figures on the CPU (tests/test_connect_definition_cpu.py) -- never from the device's.  The cached forms are handed
`lsub` and `pad = eye label + 1` the way the device passes fill them; where the stored label differs from the tree's the definition
follows the stored one, so the device's answer has to move exactly as the definition predicts.

Out-of-range cached label words are NOT fed to the GPU: a broken guard would read past the Gamma table, and this suite does not go
looking for faults (the host refuses an `lsub` that is no label before anything is launched; connect_families.check_ranges).

SPCBPT_UNIT_REPORT=1 prints every figure without stopping at the first bar missed, as in tests/test_gpu_units.py."""
import os

import numpy as np
import pytest

from tests import connect_families as CF
from tests import connect_ref as R

pytestmark = pytest.mark.gpu
SOFT = bool(os.environ.get("SPCBPT_UNIT_REPORT"))
CONNECT, EYE_STEP, SKY_MISS = 6, 7, 8
WORLDS = ("cornell", "flagged", "courtyard")
FORM = dict(reference=0, cached=1, cached_plain=2)      # SPCBPT_UNIT_FORM_* (api.UNIT_FORMS: test_what_no_launcher_would_pick_is_refused compares)


@pytest.fixture(scope="module", params=WORLDS)
def world(request, gpu, pkg, ob):
    w = CF.build_world(pkg, ob, request.param)
    r = pkg.Renderer(w["scene"], 0)
    cam = w["scene"].camera
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w["W"] / w["H"])
    r.resize(w["W"], w["H"])
    if w["env"] is not None:
        r.set_environment(w["env"]["rgba"], w["env"]["center"], w["env"]["radius"])
    r.set_subspace(*w["tup"])
    w["r"] = r
    return w


def dev_connect(w, f, form):
    n = len(f["a"])
    words = np.zeros((n, 52), np.uint32)
    words[:, :25] = f["a"].view(np.uint32).reshape(n, 25)
    words[:, 25:49] = f["b"].view(np.uint32).reshape(n, 24)
    words[:, 49] = FORM[form]
    words[:, 50] = f["lsub"]
    out = w["r"].unit(CONNECT, words, 5)
    g = out.view(np.float32)
    return g[:, :3].copy(), g[:, 3].copy(), out[:, 4].copy()


def dev_eye_step(w, ob, f, form):
    rec = f["rec"].copy()
    rec["pad"][:, 0] = FORM[form]
    rec["pad"][:, 1] = f["lsub"]
    out = w["r"].unit(EYE_STEP, rec.view(np.uint32).reshape(len(rec), -1), 40)
    return out.view(ob.EYE_STEP_OUT_DTYPE).reshape(-1)


def dev_sky_miss(w, s, form):
    n = len(s["last"])
    words = np.zeros((n, 34), np.uint32)
    words[:, :25] = s["last"].view(np.uint32).reshape(n, 25)
    words[:, 25:28] = s["next_flux"].view(np.uint32)
    words[:, 28] = s["next_single_pdf"].view(np.uint32)
    words[:, 29:32] = s["dirs"].view(np.uint32)
    words[:, 32] = FORM[form]
    words[:, 33] = s["lsub"]
    out = w["r"].unit(SKY_MISS, words, 6)
    g = out.view(np.float32)
    return g[:, :3].copy(), g[:, 3].copy(), out[:, 4].astype(np.int64)


def hold(fails, problems):
    for _, m in fails:
        problems.append(m)


def finish(problems):
    if problems and SOFT:
        print("\n".join(["MISSED:"] + problems))
        return
    assert not problems, "\n".join(problems)


def audit_device_connect(w, f, form, name):
    rgb, wt, null = dev_connect(w, f, form)
    res = R.audit_connect(w["scene"], w["tup"], f["a"], f["b"], rgb, wt, got_null=null, judge_value=f["judge_value"], form=form, lsub=f["lsub"],
                          project_pdf=w["project_pdf"], extent=w["extent"])
    return res, rgb, wt, null, R.judge(res, len(f["a"]), f"device, {w['which']}, {name}, {form}", depth=f["a"]["depth"])


def test_every_connection_family_in_every_legal_form(world):
    w = world
    fams = CF.connect_families(w)
    problems, got = [], {}
    for name, f in fams.items():
        for form in f["forms"]:
            res, rgb, wt, null, fails = audit_device_connect(w, f, form, name)
            hold(fails, problems)
            got[name, form] = (rgb, wt, null, res["_def"])
            if name == "grazing":     # on EVERY record: the exact zeros are exact zeros; null => value 0; the flag is the definition's sign test
                D = res["_def"]
                z = (f["sa"] == 0) | (f["sb"] == 0)
                if not ((rgb[z] == 0).all() and (rgb[null != 0] == 0).all()):
                    problems.append(f"{name}, {form}: a grazing pair with an exact zero cosine, or one the null test skips, has a value")
                if len(res["connect: null flag"].err) != len(f["a"]):      # +-1e-3, +-1e-6 and exact zeros: none within an ulp of the sign change
                    problems.append(f"{name}, {form}: {len(f['a']) - len(res['connect: null flag'].err)} grazing records within an ulp of the sign change")
                if not ((null != 0) == D["null"]).all():
                    problems.append(f"{name}, {form}: the null flag differs from the definition's sign test on {int(((null != 0) != D['null']).sum())} records")
            if name == "zero-handled Q cells":
                z = f["zero_over_zero"]
                if not (np.isnan(wt[z]).all() and (rgb[z] == 0).all()):
                    problems.append(f"{name}, {form}: 0 / 0 is not rejected")
    # the timed path is the one under test: with a wrong `lsub` / `pad` label a cached form moves away from its own answer on the
    # trees' labels -- to where the definition says (the audit above has judged both)
    for form in fams["chain"]["forms"]:
        if form == "reference":
            continue
        own, other = got["chain", form], got["stored labels differ from the trees'", form]
        a, b = fams["chain"]["a"], fams["chain"]["b"]
        reads = ((a["depth"] >= 2) | (b["depth"] > 0)) & np.isfinite(own[1]) & (own[1] > 0) & (own[1] < 1)
        moved = own[1][reads] != other[1][reads]
        print(f"device, {w['which']}, {form}: a wrong stored label moves the weight on {moved.mean():.4f} of the records that read one")
        if not moved.mean() > 0.9:
            problems.append(f"{form}: the stored labels are not what the weight reads ({moved.mean():.3f} moved)")
    finish(problems)


def test_every_eye_step_family_in_every_legal_form(world, ob):
    w = world
    problems = []
    fams = CF.eye_step_families(w)
    got = {}
    for name, f in fams.items():
        for form in f["forms"]:
            out = dev_eye_step(w, ob, f, form)
            got[name, form] = out
            res = R.audit_eye_step(w["scene"], w["tup"], f["rec"], out, form=form, lsub=f["lsub"], got_lsub=out["pad"])
            res.pop("_def")
            res.update(R.audit_emitter_hit(w["scene"], w["tup"], f["rec"], out, form=form, lsub=f["lsub"], env=w["env"]))
            res.pop("_def")
            hold(R.judge(res, len(f["rec"]), f"device, {w['which']}, eye step, {name}, {form}", depth=f["rec"]["last"]["depth"]), problems)
    for form in fams["walk"]["forms"]:
        if form == "reference":
            continue
        own, other = got["walk", form], got["stored lsub differs from the tree's", form]
        surf = (own["kind"] == 1) & (other["kind"] == 1) & (fams["walk"]["rec"]["last"]["depth"] >= 2)
        moved = (own["mid"]["rmis3"][surf] != other["mid"]["rmis3"][surf]).any(1)
        print(f"device, {w['which']}, {form}: a wrong lsub moves rmis3 on {moved.mean():.4f} of the vertices behind depth 2")
        if not (surf.sum() > 200 and moved.mean() > 0.9):
            problems.append(f"{form}: the previous vertex's lsub is not what rmis3 reads ({moved.mean():.3f} moved)")
    finish(problems)


def test_sky_miss_in_both_forms(world, pkg):
    w = world
    if w["env"] is None:
        with pytest.raises(pkg.SpcbptError, match=r"\(-5\)"):   # no sky: SPCBPT_ERR_STATE, as before
            w["r"].unit(SKY_MISS, np.zeros((1, 34), np.uint32), 6)
        return
    s = CF.sky_miss_family(w)
    problems = []
    got = {}
    for form in ("reference", "cached"):
        rgb, wt, label = dev_sky_miss(w, s, form)
        got[form] = (rgb, wt)
        res = R.audit_sky_miss(w["scene"], w["tup"], s["last"], s["next_flux"], s["next_single_pdf"], s["dirs"], rgb, wt, label, w["env"], form=form, lsub=s["lsub"])
        hold(R.judge(res, len(s["last"]), f"device, courtyard, sky miss, {form}", depth=s["last"]["depth"]), problems)
    words = np.zeros((4, 32), np.uint32)          # today's 32-word record: the reference form, bit for bit
    n = 4
    words[:, :25] = s["last"][:n].view(np.uint32).reshape(n, 25); words[:, 25:28] = s["next_flux"][:n].view(np.uint32)
    words[:, 28] = s["next_single_pdf"][:n].view(np.uint32); words[:, 29:32] = s["dirs"][:n].view(np.uint32)
    old = w["r"].unit(SKY_MISS, words, 6).view(np.float32)
    assert np.array_equal(old[:, :4].view(np.uint32), np.concatenate([got["reference"][0][:n], got["reference"][1][:n, None]], 1).view(np.uint32))
    assert (s["last"]["depth"] == 0).sum() > 100 and (s["last"]["depth"] >= 2).sum() > 500 and (got["cached"][0] != 0).any(1).mean() > 0.5
    # the two forms against each other (the family carries the tree's own lsub): the full difference at the bar
    D = res["_def"]
    idx = np.arange(len(s["last"]))
    cross = {"sky value": R.Check("sky value", idx, R.rel(got["cached"][0], got["reference"][0]), D["kappa"]["value"]),
             "sky weight": R.Check("sky weight", idx, R.rel(got["cached"][1], got["reference"][1]), D["kappa"]["w"])}
    same = (got["cached"][0].view(np.uint32) == got["reference"][0].view(np.uint32)).all(1) & (got["cached"][1].view(np.uint32) == got["reference"][1].view(np.uint32))
    print(f"device, courtyard, sky miss: reference / cached bit-equal on {same.mean():.4f} of {len(same)} records")
    hold(R.judge(cross, len(idx), "device, courtyard, sky miss, reference against cached", depth=s["last"]["depth"]), problems)
    finish(problems)


def test_the_three_forms_agree_on_the_trees_own_labels(world, ob):
    """Records that are legal in every form of their scene and carry the trees' own labels: the forms against each other, their full
    difference held to the bar (BARS + C kappa, as one answer against the definition) and not to bit equality; the bit-equal share
    is printed."""
    w = world
    problems = []
    for name, f in CF.connect_families(w).items():
        if not f["tree_labels"] or "reference" not in f["forms"]:
            continue
        D = R.connect(w["scene"], w["tup"], f["a"], f["b"], form="reference", project_pdf=w["project_pdf"], extent=w["extent"])
        outs = {form: dev_connect(w, f, form) for form in f["forms"]}
        ref = outs["reference"]
        jv = np.ones(len(f["a"]), bool) if f["judge_value"] is None else f["judge_value"]
        for form in f["forms"][1:]:
            o = outs[form]
            same = (ref[0].view(np.uint32) == o[0].view(np.uint32)).all(1) & (ref[1].view(np.uint32) == o[1].view(np.uint32))
            print(f"device, {w['which']}, {name}: reference / {form} bit-equal on {same.mean():.4f} of {len(same)} records")
            idx = np.nonzero(jv)[0]
            res = {"connect value": R.Check("connect value", idx, R.rel(o[0], ref[0])[jv], D["k_through"][jv]),
                   "connect weight": R.Check("connect weight", idx, R.rel(o[1], ref[1])[jv], D["k_w"][jv]),
                   "connect: null flag": R.Check("connect: null flag", np.arange(len(same)), (o[2] != ref[2]).astype(float))}
            hold(R.judge(res, len(same), f"device, {w['which']}, {name}, reference against {form}", depth=f["a"]["depth"]), problems)
    f = CF.eye_step_families(w)["walk"]
    outs = {form: dev_eye_step(w, ob, f, form) for form in f["forms"]}
    full = R.audit_eye_step(w["scene"], w["tup"], f["rec"], outs["reference"])["_def"]
    sel, kap = full["sel"], full["kappa"]
    for form in f["forms"][1:]:
        o, ref = outs[form], outs["reference"]
        if not (np.array_equal(o["kind"], ref["kind"]) and np.array_equal(o["seed"], ref["seed"]) and np.array_equal(o["done"], ref["done"])):
            problems.append(f"eye step, reference against {form}: kind, seed or done differ")
            continue
        a, b = o.copy(), ref.copy()
        a["pad"] = b["pad"] = 0                                     # (the cached forms report lsub there)
        print(f"device, {w['which']}, eye step: reference / {form} bit-equal on {np.mean([x.tobytes() == y.tobytes() for x, y in zip(a, b)]):.4f} of {len(a)} records")
        res = {}
        for check, field, k in (("eye flux", "flux", "flux"), ("eye single_pdf", "single_pdf", "single_pdf"), ("eye rmis3", "rmis3", "rmis3")):
            res[check] = R.Check(check, sel, R.rel(o["mid"][field][sel], ref["mid"][field][sel]), kap[k])
        res["eye pdf"] = R.Check("eye pdf", sel, R.rel(o["mid"]["pdf"][sel], ref["mid"]["pdf"][sel]), kap["single_pdf"])
        res["eye last_normal_projection"] = R.Check("eye last_normal_projection", sel, np.abs(o["mid"]["last_normal_projection"][sel].astype(np.float64)
                                                                                         - ref["mid"]["last_normal_projection"][sel]), kap["lnp"])
        res["next flux"] = R.Check("next flux", sel, R.rel(o["next_flux"][sel], ref["next_flux"][sel]), kap["next_flux"])
        alive = ref["done"][sel] == 0
        res["next single_pdf"] = R.Check("next single_pdf", sel[alive], R.rel(o["next_single_pdf"][sel][alive], ref["next_single_pdf"][sel][alive]), kap["next_single_pdf"][alive])
        res["eye: position, normal, colour, integers"] = R.Check("eye: position, normal, colour, integers", sel, np.array(
            [any(x[k].tobytes() != y[k].tobytes() for k in ("position", "normal", "color", "last_position", "material_id", "depth", "last_zone_id"))
             for x, y in zip(o["mid"][sel], ref["mid"][sel])], float))
        res["eye: subspace label"] = R.Check("eye: subspace label", sel, (o["mid"]["subspace_id"][sel] != ref["mid"]["subspace_id"][sel]).astype(float))
        em = np.nonzero(ref["kind"] == 2)[0]
        res["emitter radiance"] = R.Check("emitter radiance", em, R.rel(o["emit"][em], ref["emit"][em]), np.zeros(len(em)))
        hold(R.judge(res, len(a), f"device, {w['which']}, eye step, reference against {form}"), problems)
    finish(problems)


def test_a_record_as_the_tests_build_it_today_is_the_reference_form(world):
    """form word 0, today's in_words / out_words and zero pad words: bit for bit what an explicit `reference` returns"""
    w = world
    f = CF.connect_families(w)["chain"]
    n = 512
    words = np.zeros((n, 52), np.uint32)
    words[:, :25] = f["a"][:n].view(np.uint32).reshape(n, 25)
    words[:, 25:49] = f["b"][:n].view(np.uint32).reshape(n, 24)
    words[:, 48] &= np.uint32(R.LV_DIRECTION | R.LV_LAST_DIRECTION)          # pad as an oracle cache carries it: flags only
    old = w["r"].unit(CONNECT, words, 4)
    words[:, 50] = 777                                                       # (lsub is not read by the reference form)
    new = w["r"].unit(CONNECT, words, 5)
    assert old.shape == (n, 4) and np.array_equal(old, new[:, :4])


def test_what_no_launcher_would_pick_is_refused(world, pkg):
    w = world
    r = w["r"]
    assert pkg.api.UNIT_FORMS == FORM
    f = CF.connect_families(w)["chain"]
    words = np.zeros((2, 52), np.uint32)
    words[:, :25] = f["a"][:2].view(np.uint32).reshape(2, 25)
    words[:, 25:49] = f["b"][:2].view(np.uint32).reshape(2, 24)
    step = CF.eye_step_families(w)["walk"]["rec"][:2].copy()

    def refused(code, what, op, rec, out_words):
        with pytest.raises(pkg.SpcbptError, match=rf"\({code}\).*{what}"):
            r.unit(op, rec, out_words)
    if w["which"] != "cornell":       # cached_plain on a general scene
        words[:, 49] = pkg.api.UNIT_FORM_CACHED_PLAIN
        refused(-5, "general", CONNECT, words, 5)
        step["pad"][:, 0] = pkg.api.UNIT_FORM_CACHED_PLAIN
        refused(-5, "general", EYE_STEP, step.view(np.uint32).reshape(2, -1), 40)
    words[:, 49] = 3
    refused(-1, "unknown form", CONNECT, words, 5)
    words[:, 49], words[:, 50] = pkg.api.UNIT_FORM_CACHED, pkg.NUM_SUBSPACE      # never launched: the host refuses a word that is no label
    refused(-1, "no.* label", CONNECT, words, 5)
    if w["env"] is not None:
        sky = np.zeros((1, 34), np.uint32)
        sky[:, 32] = pkg.api.UNIT_FORM_CACHED_PLAIN
        refused(-1, "SKY_MISS", SKY_MISS, sky, 6)
    # a classifier with a direction node: labels depend on the viewing direction, nothing caches them
    et, lt, q, cmf = w["tup"]
    et2 = et.copy()
    et2[1]["type"] = 2
    r.set_subspace(et2, lt, q, cmf)
    try:
        words[:, 49], words[:, 50] = pkg.api.UNIT_FORM_CACHED, 0
        refused(-5, "direction nodes", CONNECT, words, 5)
        step["pad"][:, 0] = pkg.api.UNIT_FORM_CACHED
        refused(-5, "direction nodes", EYE_STEP, step.view(np.uint32).reshape(2, -1), 40)
        if w["env"] is not None:
            sky = np.zeros((1, 34), np.uint32)
            sky[:, 32] = pkg.api.UNIT_FORM_CACHED
            refused(-5, "direction nodes", SKY_MISS, sky, 6)
            sky[:, 32] = 3
            refused(-1, "unknown form", SKY_MISS, sky, 6)
        step["pad"][:, 0] = 3
        refused(-1, "unknown form", EYE_STEP, step.view(np.uint32).reshape(2, -1), 40)
        words[:, 49] = pkg.api.UNIT_FORM_REFERENCE
        assert r.unit(CONNECT, words, 5).shape == (2, 5)                        # the reference form runs on any tree
    finally:
        r.set_subspace(*w["tup"])


def test_the_mesh_light_arm_of_the_emitter_hit_against_the_definition(gpu, pkg, ob):
    """`L.type == 2` in eye_emitter_hit: the hit triangle's own normal, the patch's label, pdf 1 / (area n_lights).  The reference has
    no mesh lights and the oracle restates none (its binding refuses such a scene), so here the device ALONE is held to the
    definition, at the bars the oracle set for the quad light: four levels of the device's own walk through the Cornell box under
    the sphere lamp, in the two forms a general scene has, and the forms against each other."""
    scene = pkg.scenes.cornell_sphere_lamp()
    W, H = 64, 36
    r = pkg.Renderer(scene, 0)
    cam = scene.camera
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
    r.resize(W, H)
    tup = CF.audit_tuple(pkg, scene)
    r.set_subspace(*tup)
    w = dict(r=r, tup=tup, which="lamp")
    rec = CF.camera_records(pkg, ob, scene, 4 * CF.N_CAMERA, np.random.default_rng(21), W / H)
    steps = []
    for level in range(1, 5):
        out = dev_eye_step(w, ob, dict(rec=rec, lsub=np.zeros(len(rec), np.int64)), "reference")
        steps.append(rec)
        go = (out["kind"] == 1) & (out["done"] == 0)
        nxt = np.zeros(int(go.sum()), ob.EYE_STEP_IN_DTYPE)
        nxt["last"] = out["mid"][go]; nxt["next_flux"] = out["next_flux"][go]; nxt["next_single_pdf"] = out["next_single_pdf"][go]
        nxt["seed"] = out["seed"][go]; nxt["dir"] = out["dir"][go]
        rec = nxt
    rec = np.concatenate(steps)
    f = dict(rec=rec, lsub=CF.own_lsub(w, rec["last"]))
    problems, outs = [], {}
    for form in ("reference", "cached"):
        out = outs[form] = dev_eye_step(w, ob, f, form)
        res = R.audit_eye_step(scene, tup, rec, out, form=form, lsub=f["lsub"], got_lsub=out["pad"])
        res.pop("_def")
        res.update(R.audit_emitter_hit(scene, tup, rec, out, form=form, lsub=f["lsub"]))
        kap = res.pop("_def")["kappa"]["value"]
        hold(R.judge(res, len(rec), f"device, sphere lamp, eye step, {form}", depth=rec["last"]["depth"]), problems)
    hit = outs["reference"]["kind"] == 2
    # enough hits to fill the 99.9 % quantile's neighbourhood, a third of them behind depth 2, where light_hit runs (the lamp fills about
    # one percent of the view: 162 and 56 of these 12 288 camera paths)
    assert hit.sum() > 100 and (hit & (rec["last"]["depth"] >= 1)).sum() > 30, (int(hit.sum()), int((hit & (rec["last"]["depth"] >= 1)).sum()))
    assert (outs["reference"]["emit"][hit] != 0).any(1).all() and np.array_equal(outs["reference"]["kind"], outs["cached"]["kind"])
    em = np.nonzero((outs["reference"]["kind"] == 2) | (outs["reference"]["kind"] == 3))[0]
    cross = {"emitter radiance": R.Check("emitter radiance", em, R.rel(outs["cached"]["emit"][em], outs["reference"]["emit"][em]), kap)}
    hold(R.judge(cross, len(rec), "device, sphere lamp, reference against cached"), problems)
    step = rec[:2].copy()
    step["pad"][:, 0] = FORM["cached_plain"]                    # a mesh light makes the scene general
    with pytest.raises(pkg.SpcbptError, match=r"\(-5\).*general"):
        r.unit(EYE_STEP, step.view(np.uint32).reshape(2, -1), 40)
    finish(problems)
