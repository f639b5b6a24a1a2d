"""The float64 definition of the eye side (tests/connect_ref.py) on the CPU: the check of the check.

1. The ORACLE's connect / eye_step outputs pass the audit on every record family it can express (tests/connect_families.py; the
   oracle classifies by descent, so it speaks for the `reference` form only): the definition's formulas are the reference's.  For
   the sky miss the oracle has one number, the rmis::light_hit_env weight of an escaped camera path (orc_debug_env_partition): it
   passes too.  Every run prints the figures connect_ref.BARS were derived from (run with -s); the last test of this part holds the
   table to them.
2. The audit sees what it is for: one seeded mistake at a time, applied to about 0.3 % of the records of a passing family, makes
   exactly its own check fail, and the failure names corrupted records and no other."""
import numpy as np
import pytest

from tests import connect_families as CF
from tests import connect_ref as R

WORLDS = ("cornell", "flagged", "courtyard")
_cache = {}


def world(pkg, ob, which):
    if which not in _cache:
        _cache[which] = CF.build_world(pkg, ob, which)
    return _cache[which]


def oracle_connect(w, f, rgb=None, wt=None, **kw):
    if rgb is None:
        rgb, wt = w["o"].connect(f["a"], f["b"])
    return R.audit_connect(w["scene"], w["tup"], f["a"], f["b"], rgb, wt, judge_value=f["judge_value"], form="reference",
                           project_pdf=w["project_pdf"], extent=w["extent"], **kw), rgb, wt


def oracle_eye(w, f, out=None):
    out = w["o"].eye_step(f["rec"]) if out is None else out
    res = R.audit_eye_step(w["scene"], w["tup"], f["rec"], out)
    res.pop("_def")
    res.update(R.audit_emitter_hit(w["scene"], w["tup"], f["rec"], out, env=w["env"]))
    res.pop("_def")
    return res, out


FIGURES = {}      # check: [largest 99.9 % quantile, largest maximum] of the oracle over everything the tests below ran


def _note(res):
    for name, (q, m, _) in R.figures(res).items():
        cur = FIGURES.setdefault(name, [0.0, 0.0])
        cur[0], cur[1] = max(cur[0], q), max(cur[1], m)


@pytest.mark.parametrize("which", WORLDS)
def test_the_oracle_passes_the_audit(pkg, ob, which):
    w = world(pkg, ob, which)
    fams = CF.connect_families(w)
    for name, f in fams.items():
        res, rgb, wt = oracle_connect(w, f)
        _note(res)
        fails = R.judge(res, len(f["a"]), f"oracle, {which}, {name}", depth=f["a"]["depth"])
        assert not fails, "\n".join(m for _, m in fails)
        D, a, b = res["_def"], f["a"], f["b"]
        live = (rgb != 0).any(1)
        if name == "chain":       # a.depth == 1 (no eye-side weight) against depth >= 2; b.depth == 0 and > 0
            assert (a["depth"] == 1).sum() > 500 and (a["depth"] >= 3).sum() > 100 and (b["depth"] == 0).sum() > 500 and live.mean() > 0.3
            assert (a["rmis3"][a["depth"] == 1] == 0).all()
        if name == "emitter vertex from the front and from behind":
            assert (live & (D["s_b"] > 0)).sum() > 300 and (D["s_b"] < 0).sum() > 300 and not live[D["s_b"] < 0].any()
        if name == "grazing":     # the exact zeros are exact zeros, on the oracle as well
            z = (f["sa"] == 0) | (f["sb"] == 0)
            assert z.sum() > 500 and ((D["s_a"] == 0) == (f["sa"] == 0)).all() and ((D["s_b"] == 0) == (f["sb"] == 0)).all()
            assert (rgb[z] == 0).all() and (rgb[D["null"]] == 0).all()
            for v in (1e-3, -1e-3, 1e-6, -1e-6):
                assert np.allclose(D["s_a"][f["sa"] == v], v, rtol=0.2) and np.allclose(D["s_b"][f["sb"] == v], v, rtol=0.2)
        if name == "short connections":   # the rejection of ISINVALIDVALUE on both sides of its threshold
            with np.errstate(all="ignore"):
                top = np.nanmax(D["through"] * wt[:, None].astype(np.float64), 1)
            r = np.linalg.norm(a["position"].astype(np.float64) - b["position"], axis=1)
            assert r.min() < 1.2 * R.SCENE_EPSILON and (top > 1e5).sum() > 50 and ((top < 1e5) & (top > 1e3)).sum() > 50
            assert (rgb[top > 1.001e5] == 0).all() and (rgb[(top < 0.999e5) & (top > 0)] != 0).any(1).all()
        if name == "zero-handled Q cells":
            z = f["zero_over_zero"]
            assert z.sum() > 50 and np.isnan(wt[z]).all() and np.isnan(D["w"][z]).all() and (rgb[z] == 0).all()      # 0 / 0 is rejected
            zw = (b["subspace_id"] == CF.ZERO_LIGHT) & ~z & ~D["sky"]
            assert zw.sum() > 300 and (wt[zw & ~np.isnan(wt)] == 0).all() and (rgb[zw] == 0).all()
        if name == "sky directions":
            assert D["sky"].all() and (D["null"]).sum() > 300 and live.sum() > 300
        if name == "light vertices lit straight by the sky":
            assert ((b["pad"] & np.uint32(R.LV_LAST_DIRECTION)) != 0).all() and live.sum() > 200
    for name, f in CF.eye_step_families(w).items():
        if "reference" not in f["forms"]:
            continue
        res, out = oracle_eye(w, f)
        _note(res)
        fails = R.judge(res, len(f["rec"]), f"oracle, {which}, eye step, {name}", depth=f["rec"]["last"]["depth"])
        assert not fails, "\n".join(m for _, m in fails)
        if name == "walk":
            d = out["mid"]["depth"][out["kind"] == 1]
            assert (d == 1).sum() > 500 and (d == 2).sum() > 200 and (d >= 3).sum() > 100 and len(res["emitter radiance"].err) > 10
    print(f"oracle, {which}: largest 99.9 % quantile / maximum over c kappa so far: " + "; ".join(f"{k}: {q:.3g} / {m:.3g}" for k, (q, m) in sorted(FIGURES.items())))


def _oracle_sky_miss(pkg, ob):
    """The oracle's rmis::light_hit_env weights of camera paths that leave the courtyard after 1 .. 4 surface vertices, by the very
    function the renderers call (orc_debug_env_partition); it returns no value for them."""
    w = world(pkg, ob, "courtyard")
    total = 0
    for depth in (1, 2, 3, 4):
        wo, _, ev, lv = w["o"].env_partition(depth, 1500, vertices=True)
        dirs = -lv[:, 0]["normal"]
        keep = CF.clear_of_sky_borders(w, dirs)
        last, dirs, got_w, label = ev[keep, 0], dirs[keep], wo[keep, 1], lv[keep, 0]["subspace_id"]
        one = np.ones((len(last), 3), np.float32)
        res = R.audit_sky_miss(w["scene"], w["tup"], last, one, one[:, 0], dirs, None, got_w, label, w["env"])
        res.pop("_def")
        _note(res)
        fails = R.judge(res, len(last), f"oracle, courtyard, sky miss after {depth} vertices", depth=last["depth"])
        assert not fails, "\n".join(m for _, m in fails)
        assert (last["depth"] == depth).all()
        total += len(last)
    assert total > 3000


def test_the_oracles_sky_miss_weight_passes_the_audit(pkg, ob):
    _oracle_sky_miss(pkg, ob)


def test_the_bars_are_the_stated_margin_over_the_oracle(pkg, ob):
    """connect_ref.BARS: 4 x the oracle's largest 99.9 % quantile (floored at 2e-6) and 4 x its largest maximum, to two digits; the
    sky-miss value, which the oracle has no entry point for, takes the bars of the sky-miss weight (connect_ref says why)."""
    if "connect value" not in FIGURES:
        for which in WORLDS:
            test_the_oracle_passes_the_audit(pkg, ob, which)
    if "sky weight" not in FIGURES:
        _oracle_sky_miss(pkg, ob)
    assert set(FIGURES) | {"sky value"} == set(R.BARS)
    for name, (q, m) in FIGURES.items():
        bar, hard = R.BARS[name]
        want_bar, want_hard = max(4.0 * q, 2e-6), max(4.0 * m, 4.0 * q, 2e-6)
        assert R.BARS["sky value"] == R.BARS["sky weight"]
        assert 0.94 * want_bar <= bar <= 1.06 * want_bar and 0.94 * want_hard <= hard <= 1.06 * want_hard, (name, (bar, hard), (want_bar, want_hard))


# ---------------------------------------------------------------------------------------------------------------- corruptions
def f32(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x, np.float64).astype(np.float32)


@pytest.fixture(scope="module")
def chain(pkg, ob):
    w = world(pkg, ob, "cornell")
    f = CF.connect_families(w, n=12000)["chain"]
    res, rgb, wt = oracle_connect(w, f)
    assert not R.judge(res, len(f["a"]), "oracle", report=lambda s: None)
    return dict(w=w, f=f, rgb=rgb, wt=wt, D=res["_def"])


# mistake: (the records it can show on, the checks that must fail -- and no other)
CONNECT_BUGS = {
    "Gamma indices transposed": (lambda a, b, D: np.ones(len(a), bool), {"connect weight"}),
    "CONNECTION_N dropped": (lambda a, b, D: a["depth"] >= 2, {"connect weight"}),
    "last_normal_projection dropped from LL_pdf": (lambda a, b, D: (a["depth"] >= 2) & (b["depth"] > 0), {"connect weight"}),
    "1 / r^2 -> 1 / r": (lambda a, b, D: np.ones(len(a), bool), {"connect value"}),
    "rr dropped": (lambda a, b, D: np.ones(len(a), bool), {"connect weight"}),
    "fb one-sided test flipped": (lambda a, b, D: (b["depth"] == 0) & (D["s_b"] > 0), {"connect value"}),
    "pdf_A taken from the wrong vertex": (lambda a, b, D: b["depth"] > 0, {"connect weight"}),
}


def _judge_corrupted(res, n, what, rows, expected):
    fails = R.judge(res, n, what, report=lambda s: None)
    assert R.failed_checks(fails) == sorted(expected), [m for _, m in fails]
    for f in fails:
        name, msg = f
        assert msg.startswith(f"{what}: {name}: ") and "first: (" in msg, msg
        assert np.isin(f.records, rows).all(), (name, f.records[~np.isin(f.records, rows)][:5])       # names corrupted records and no other
        assert np.isin(rows, f.records).mean() >= 0.9, (name, float(np.isin(rows, f.records).mean()))
        named = [int(s.split(",")[0]) for s in msg.split("first: (")[1].split("), (")]
        assert all(i in rows for i in named), msg


def _pick(ok, n, rng):
    rows = np.nonzero(ok)[0]
    k = int(round(0.003 * n))
    assert len(rows) >= k >= 10, (len(rows), k)
    return np.sort(rng.choice(rows, k, replace=False))


@pytest.mark.parametrize("bug", list(CONNECT_BUGS))
def test_a_mistake_in_the_connection_fails_exactly_its_own_check(chain, bug):
    w, f, D = chain["w"], chain["f"], chain["D"]
    where, expected = CONNECT_BUGS[bug]
    a, b, n = f["a"], f["b"], len(f["a"])
    Db = R.connect(w["scene"], w["tup"], a, b, form="reference", extent=w["extent"], bug=bug, kappa=False)
    with np.errstate(all="ignore"):
        moved = np.maximum(np.abs(Db["w"] - D["w"]) / np.abs(D["w"]), np.abs(Db["through"] - D["through"]).max(1) / np.abs(D["through"]).max(1))
        top = np.abs(D["through"] * D["w"][:, None]).max(1)
    ok = where(a, b, D) & (moved > 1e-2) & (top > 0) & (top < 1e4) & (2 * np.maximum(D["k_w"], D["k_through"]) < 1e-4) & (chain["rgb"] != 0).any(1)
    rows = _pick(ok, n, np.random.default_rng(sum(map(ord, bug))))
    rgb, wt = chain["rgb"].copy(), chain["wt"].copy()
    wt[rows] = f32(Db["w"][rows])
    rgb[rows] = f32(R.value_of(Db["through"][rows], wt[rows]))
    res, _, _ = oracle_connect(w, f, rgb, wt)
    _judge_corrupted(res, n, bug, rows, expected)


@pytest.mark.parametrize("field", ["rgb", "weight"])
def test_a_relative_perturbation_of_1e_3_of_a_connection_output_is_seen(chain, field):
    w, f, D = chain["w"], chain["f"], chain["D"]
    n = len(f["a"])
    ok = (chain["rgb"] != 0).any(1) & (2 * np.maximum(D["k_w"], D["k_through"]) < 1e-4)
    rows = _pick(ok, n, np.random.default_rng(len(field)))
    rgb, wt = chain["rgb"].copy(), chain["wt"].copy()
    if field == "rgb":
        rgb[rows] *= np.float32(1.001)
    else:
        wt[rows] *= np.float32(1.001)      # the value is no longer the throughput times the stored weight: both name it
    res, _, _ = oracle_connect(w, f, rgb, wt)
    _judge_corrupted(res, n, field, rows, {"connect value"} if field == "rgb" else {"connect value", "connect weight"})


@pytest.fixture(scope="module")
def walk(pkg, ob):
    w = world(pkg, ob, "cornell")
    f = CF.eye_step_families(w)["walk"]
    res, out = oracle_eye(w, f)
    assert not R.judge(res, len(f["rec"]), "oracle", report=lambda s: None)
    full = R.audit_eye_step(w["scene"], w["tup"], f["rec"], out)
    return dict(w=w, f=f, out=out, full=full)


EYE_BUGS = {
    # mistake: (field of the definition it moves, the output fields rewritten from it, expected checks)
    "Gamma indices transposed": ("rmis3", {"eye rmis3"}),
    "CONNECTION_N dropped": ("rmis3", {"eye rmis3"}),
    "last_normal_projection dropped from LL_pdf": ("rmis3", {"eye rmis3"}),
    "1 / r^2 -> 1 / r": ("flux", {"eye flux", "eye single_pdf"}),       # pdf_G enters both; the stored pdf is rebuilt from the stored single_pdf
    "rr dropped": ("next_single_pdf", {"next single_pdf"}),
}


@pytest.mark.parametrize("bug", list(EYE_BUGS))
def test_a_mistake_in_the_eye_step_fails_exactly_its_own_check(walk, bug):
    w, f, out0 = walk["w"], walk["f"], walk["out"]
    key, expected = EYE_BUGS[bug]
    base, kap, sel = walk["full"]["_def"]["base"], walk["full"]["_def"]["kappa"], walk["full"]["_def"]["sel"]
    wrong = R.audit_eye_step(w["scene"], w["tup"], f["rec"], out0, bug=bug)["_def"]["base"]
    with np.errstate(all="ignore"):
        moved = np.abs(wrong[key] - base[key]) / np.abs(base[key])
        moved = moved.max(-1) if moved.ndim > 1 else moved
    ok = (moved > 1e-2) & (2 * kap[key] < 1e-4) & np.isfinite(moved)
    if key == "next_single_pdf":
        ok &= out0["done"][sel] == 0
    k = _pick(ok, len(f["rec"]), np.random.default_rng(sum(map(ord, bug))))
    rows = sel[k]
    out = out0.copy()
    if key == "rmis3":
        out["mid"]["rmis3"][rows] = f32(wrong["rmis3"][k])
    elif key == "flux":
        out["mid"]["flux"][rows] = f32(wrong["flux"][k]); out["mid"]["single_pdf"][rows] = f32(wrong["single_pdf"][k])
        out["mid"]["pdf"][rows] = f["rec"]["last"]["pdf"][rows] * out["mid"]["single_pdf"][rows]
    else:
        out["next_single_pdf"][rows] = f32(wrong["next_single_pdf"][k])
    res, _ = oracle_eye(w, f, out)
    _judge_corrupted(res, len(f["rec"]), bug, rows, expected)


EYE_FIELDS = {
    "flux": {"eye flux"}, "single_pdf": {"eye single_pdf", "eye pdf"}, "pdf": {"eye pdf"}, "last_normal_projection": {"eye last_normal_projection"},
    "rmis3": {"eye rmis3"}, "next_flux": {"next flux"}, "next_single_pdf": {"next single_pdf"}, "emit": {"emitter radiance"},
}


@pytest.mark.parametrize("field", list(EYE_FIELDS))
def test_a_relative_perturbation_of_1e_3_of_an_eye_step_output_is_seen(walk, field):
    w, f, out0 = walk["w"], walk["f"], walk["out"]
    kap, sel = walk["full"]["_def"]["kappa"], walk["full"]["_def"]["sel"]
    out = out0.copy()
    rng = np.random.default_rng(len(field))
    if field == "emit":
        rows = np.nonzero((out0["kind"] == 2) & (out0["emit"] != 0).any(1))[0]           # (a few dozen emitter hits: all of them)
        out["emit"][rows] *= np.float32(1.001)
    else:
        tgt = out["mid"] if field in out["mid"].dtype.names else out
        cond = np.zeros(len(out0))
        cond[sel] = 2 * np.maximum.reduce([kap[k] for k in ("flux", "single_pdf", "rmis3", "next_flux", "next_single_pdf")])
        ok = (out0["kind"] == 1) & (cond < 1e-4) & (np.abs(np.asarray(tgt[field], np.float64).reshape(len(out), -1)).max(1) > 0)
        if field == "next_single_pdf":
            ok &= out0["done"] == 0
        if field == "last_normal_projection":
            ok &= out0["mid"]["last_normal_projection"] > 0.05      # judged absolutely, a cosine
        rows = _pick(ok, len(out), rng)
        tgt[field][rows] = tgt[field][rows] * np.float32(1.001)
    res, _ = oracle_eye(w, f, out)
    _judge_corrupted(res, len(f["rec"]), field, rows, EYE_FIELDS[field])


def test_a_flipped_null_flag_is_seen(chain):
    """the flag cleared on pairs the definition calls null (their value stays the exact zero it is): `connect: null flag` alone"""
    w, f, D = chain["w"], chain["f"], chain["D"]
    n = len(f["a"])
    ok = D["null"] & (np.abs(D["s_a"]) > 1e-3) & (np.abs(D["s_b"]) > 1e-3)
    rows = _pick(ok, n, np.random.default_rng(11))
    null = D["null"].astype(np.uint32)
    res, _, _ = oracle_connect(w, f, chain["rgb"], chain["wt"], got_null=null)
    assert not R.judge(res, n, "oracle", report=lambda s: None)
    null[rows] ^= 1
    res, _, _ = oracle_connect(w, f, chain["rgb"], chain["wt"], got_null=null)
    _judge_corrupted(res, n, "null flag", rows, {"connect: null flag"})


def test_a_wrong_returned_lsub_word_is_seen(walk):
    """EYE_STEP's returned lsub of the new vertex, off by one leaf on 0.3 % of the records: `eye: lsub label` alone"""
    w, f, out = walk["w"], walk["f"], walk["out"]
    n = len(f["rec"])
    deep = (out["kind"] == 1) & (out["mid"]["depth"] >= 2)
    own = np.zeros(n, np.int64)
    own[deep] = R.tree_labels(w["tup"][1], out["mid"]["position"][deep], out["mid"]["normal"][deep])
    res = R.audit_eye_step(w["scene"], w["tup"], f["rec"], out, form="cached", lsub=f["lsub"], got_lsub=own)
    res.pop("_def")
    assert not R.judge(res, n, "oracle", report=lambda s: None)
    rows = _pick(deep, n, np.random.default_rng(12))
    got = own.copy()
    got[rows] = CF._other(CF.LIGHT_LABELS, own[rows], np.random.default_rng(13))
    res = R.audit_eye_step(w["scene"], w["tup"], f["rec"], out, form="cached", lsub=f["lsub"], got_lsub=got)
    res.pop("_def")
    _judge_corrupted(res, n, "lsub", rows, {"eye: lsub label"})


@pytest.mark.parametrize("field", ["value", "weight", "label"])
def test_a_perturbed_sky_miss_output_is_seen(pkg, ob, field):
    """The oracle has no sky-miss record to corrupt: the definition's own answer, rounded to FP32, passes the audit, and 1e-3 on
    the value or the weight (the neighbouring label) of 0.3 % of the records fails exactly its own check."""
    w = world(pkg, ob, "courtyard")
    s = CF.sky_miss_family(w, n=6000)
    n = len(s["last"])
    args = (w["scene"], w["tup"], s["last"], s["next_flux"], s["next_single_pdf"], s["dirs"])
    base = R.audit_sky_miss(*args, np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.int64), w["env"])["_def"]
    rgb, wt = f32(base["base"]["value"]), f32(base["base"]["w"])
    label = R.env_ref.env_label(s["dirs"].astype(np.float64), 10)[0]
    res = R.audit_sky_miss(*args, rgb, wt, label, w["env"])
    assert not R.judge(res, n, "definition", report=lambda s_: None)
    ok = (rgb != 0).any(1) & (2 * np.maximum(base["kappa"]["value"], base["kappa"]["w"]) < 1e-4) & (wt < 0.999)
    rows = _pick(ok, n, np.random.default_rng(len(field)))
    if field == "value":
        rgb[rows] *= np.float32(1.001)
    elif field == "weight":
        wt[rows] *= np.float32(1.001)
    else:
        label = label.copy(); label[rows] -= 1
    res = R.audit_sky_miss(*args, rgb, wt, label, w["env"])
    _judge_corrupted(res, n, field, rows, {"value": {"sky value"}, "weight": {"sky weight"}, "label": {"sky: label"}}[field])


def test_the_oracle_refuses_a_scene_with_mesh_lights(pkg, ob):
    """The reference has no mesh lights and the oracle restates none: the `L.type == 2` arm of eye_emitter_hit has no oracle to be
    held to (tests/test_gpu_connect_definition.py audits the device alone there), and the binding says so instead of crashing."""
    with pytest.raises(ValueError, match="mesh lights"):
        ob.Oracle(pkg.scenes.cornell_sphere_lamp())
