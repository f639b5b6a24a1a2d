"""The oracle's training records against their float64 definition (tests/pretrace_ref.py), on the CPU.

Scenes cornell_box(), courtyard() with its sky, simple_room(4) (all untextured), 64 x 64; num_core 4096 at paddings 10, 3 and 2 and
4001 (a ragged last block) at padding 10; iterations 1 and 2 gathered, so that the gather's re-basing is in the data.
Tolerances: every floating-point field within pretrace_ref.BARS[field] + C_KAPPA kappa (the 99.9 % bar for 99.9 % of the records, the
hard bar for all; BARS = 4 x the oracle's own largest figures over exactly these runs, floored at 2e-6: test_bars_follow_the_oracle
holds the table to that rule); integer fields exact.  Caps: unlocated vertices <= 0.5 % of a run's records, border records (patch,
split, pixel) <= 0.1 % (LABEL_CAP), ill-conditioned records <= ILL_CAP (0.5 %) -- beyond a cap the run fails, it is never judged on
fewer records.  Each seeded mistake, applied inside the definition, must put >= 99 % of the well-conditioned records it touches outside
its own field's hard bar and must fail no check of an independent field.  The padding-2 density check is statistical: 4 standard
errors of the estimator (from its own sample variance) plus the quadrature's error (the difference of two grid resolutions)."""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import pretrace_ref as PR

W = H = 64
SCENES = ("cornell", "courtyard", "simple_room")
RUNS = ((4096, 10), (4096, 3), (4096, 2), (4001, 10))
QUAD = ((64, 8), (96, 8))      # (camera rays per axis, points per light axis) of the two quadrature resolutions


def make_scene(pkg, name):
    s = pkg.scenes
    return dict(cornell=s.cornell_box, courtyard=s.courtyard, simple_room=lambda: s.simple_room(4), lamp_floor=s.lamp_floor)[name]()


def oracle_for(ob, scene):
    o = ob.Oracle(scene)
    cam = scene.camera
    o.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
    o.resize(W, H)
    env = getattr(scene, "environment", None)
    if env is not None:
        o.set_environment(env["rgba"], env["center"], env["radius"])
    return o


def light_counts(scene):
    """(n_lights, n_drawn): every light, the sky included / the area lights the next-event candidate is drawn among"""
    n_area = len(scene.lights) + len(getattr(scene, "mesh_lights", []) or [])
    return n_area + (getattr(scene, "environment", None) is not None), n_area


def audit_records(scene, tup, paths, nodes, bug=None):
    n_lights, n_drawn = light_counts(scene)
    return PR.audit(scene, tup, PR.camera_uvw(scene.camera, W / H), W, H, paths, nodes, n_lights, n_drawn,
                    env=getattr(scene, "environment", None), bug=bug)


@pytest.fixture(scope="module")
def records(ob, pkg):
    """{(scene, num_core, padding): (scene, paths, nodes)} of the oracle, computed once"""
    out = {}
    for name in SCENES:
        scene = make_scene(pkg, name)
        for nc, pad in RUNS:
            o = oracle_for(ob, scene)
            o.pretrace(1, nc, pad); o.pretrace(2, nc, pad)
            out[name, nc, pad] = (scene,) + o.train_records()
    return out


@pytest.fixture(scope="module")
def audits(records, ob):
    return {key: audit_records(sc, (np.zeros(0),), p, n) for key, (sc, p, n) in records.items()}


@pytest.mark.parametrize("name", SCENES)
def test_oracle_records_meet_their_definition(records, audits, name):
    for nc, pad in RUNS:
        scene, paths, nodes = records[name, nc, pad]
        k = PR.check_invariants(paths, nodes, W, H, padding=pad)
        assert len(paths) > 0.2 * 2 * nc and (pad == 2) == (k.max() == 1)
        verdict = PR.judge(audits[name, nc, pad], f"oracle {name} {nc} x {pad}")
        print(f"oracle {name} {nc} x {pad}: figures (99.9 %, max, ill) = {verdict['figures']}; counted = {verdict['counts']}")
        assert verdict["ok"], verdict["fails"]


def test_bars_follow_the_oracle(audits):
    """BARS is the rule applied to these runs: 99.9 % bar = max(4 x the largest 99.9 % quantile, 2e-6), hard bar = max(4 x the largest
    maximum, the 99.9 % bar), written to two digits (rounded up, by no more than 5 %)."""
    worst = {f: [0.0, 0.0] for f in PR.FLOAT_CHECKS}
    for res in audits.values():
        for f, (q, mx, _) in PR.CR.figures(res, PR.C_KAPPA).items():
            worst[f] = [max(worst[f][0], q), max(worst[f][1], mx)]
    for f, (q, mx) in worst.items():
        bar = max(4.0 * q, 2e-6)
        hard = max(4.0 * mx, bar)
        print(f"{f}: oracle 99.9 % {q:.3g} max {mx:.3g} -> bars {bar:.3g} {hard:.3g}; table {PR.BARS[f]}")
        assert bar <= PR.BARS[f][0] <= 1.05 * bar and hard <= PR.BARS[f][1] <= 1.05 * hard, (f, q, mx, PR.BARS[f])


# the run each seeded mistake is judged on (one where it touches records: n_lights > 1 needs the sky), and the checks it may fail
BUG_RUN = {b: ("simple_room", 4096, 10) for b in PR.BUGS}
BUG_RUN["light.pdf x n_lights"] = ("courtyard", 4096, 10)
BUG_MAY_FAIL = {
    "rr dropped from the pdf arm": {"fix_pdf", "sample_pdf", "acceptance count 1 <= m <= 2 k"},   # sample_pdf* = fix_pdf + ...
    "emitter cosine dropped from nv_forward_light_pdf": set(),
    "Eval replaced by Pdf in the light arm": {"peak_pdf"},
    "light.pdf x n_lights": {"sample_pdf", "acceptance count 1 <= m <= 2 k"},
    "nodes written in eye order": {"peak_pdf"},
    "peak_pdf from the vertex one step off": {"peak_pdf"},
    "m off by one": {"sample_pdf", "acceptance count 1 <= m <= 2 k"},
}


@pytest.mark.parametrize("bug", PR.BUGS)
def test_seeded_mistakes_are_flagged(records, audits, bug):
    key = BUG_RUN[bug]
    scene, paths, nodes = records[key]
    res = audit_records(scene, (np.zeros(0),), paths, nodes, bug=bug)
    field = PR.BUG_FIELD[bug]
    verdict = PR.judge(res, f"{bug} on {key[0]}", report=lambda *_: None)
    failed = set(PR.failed_checks(verdict["fails"]))
    if field is None:
        # the light side's pdf arm past the emitter reaches no record field (pretrace_ref's docstring): the mistake
        # moves the definition's own value of it and nothing a record stores
        moved = [d["base"]["light_pdf_arm"] for d in res["_def"]["pred"].values()]
        clean = [d["base"]["light_pdf_arm"] for d in audits[key]["_def"]["pred"].values()]
        assert any((a != b).any() for a, b in zip(moved, clean)) and not failed
        return
    share, touched = PR.flagged_share(res, audits[key], field)
    print(f"{bug}: {touched} well-conditioned records of {field} touched, {share:.4f} of them outside the hard bar; failed checks {sorted(failed)}")
    assert touched > 500 and share >= 0.99, (bug, touched, share)
    assert field in failed and failed <= BUG_MAY_FAIL[bug] | {"ill-conditioned share"}, failed


@pytest.mark.parametrize("name", ("cornell", "courtyard"))
def test_claimed_next_event_density_from_first_principles(ob, pkg, name):
    """At padding 2 the records' own densities must integrate the direct light: an estimator that divides by a claimed density that is
    not the one the sample was drawn from is off by their ratio (n_lights / n_drawn = 2 on the courtyard before the claim moved)."""
    scene = make_scene(pkg, name)
    o = oracle_for(ob, scene)
    for it in range(1, 5):
        o.pretrace(it, 4096, 2)
    paths, nodes = o.train_records()
    assert ((paths["end_ind"] - paths["begin_ind"]) == 1).all()
    est, se = PR.density_estimate(paths, 4 * 4096)
    # the courtyard's quadrature runs on its coarse tessellation: the same surfaces in 20 triangles
    qscene = pkg.scenes.courtyard(n=1) if name == "courtyard" else scene
    cam = PR.camera_uvw(scene.camera, W / H)
    q = [PR.direct_light_quadrature(qscene, cam, a, b, env=getattr(scene, "environment", None)) for a, b in QUAD]
    bar = 4.0 * se + abs(q[1] - q[0])
    print(f"{name}: estimate {est:.6g} +- {se:.3g}, quadrature {q[0]:.6g} / {q[1]:.6g}, ratio {est / q[1]:.4f}, bar {bar / q[1]:.4f}")
    assert abs(est - q[1]) <= bar, (est, se, q)


def test_pretrace_refuses_a_scene_without_an_area_light(ob, pkg):
    scene = pkg.scenes.courtyard(with_quad_light=False)
    o = oracle_for(ob, scene)
    with pytest.raises(RuntimeError, match="area light"):
        o.pretrace(1, 64, 10)
    assert o.train_records_count() == 0


def test_records_without_a_sky_have_not_changed_by_a_bit(records):
    """tests/golden/pretrace_records_no_sky.json: the oracle's records of the commit before the claimed density moved (d16)"""
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pretrace_records_no_sky.json")))["oracle"]
    assert len(want) == 8
    for key, h in want.items():
        name, nc, pad = key.split()
        _, paths, nodes = records[name, int(nc), int(pad)]
        assert hashlib.sha256(paths.tobytes() + nodes.tobytes()).hexdigest() == h, key
