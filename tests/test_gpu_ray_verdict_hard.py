"""Every traversal entry point of tests/test_gpu_ray_verdict.py over the hostile scenes of tests/hard_scenes.py: trace_closest / trace_any,
trace_bench modes 0-4 (a mode whose per-ray stack does not hold 3 x bvh_depth entries must refuse), trace_pool with all of that file's
patterns and its two renderer knobs.  ZERO unexplained answers on every scene and family; K = 64, KT = 16 as everywhere.  Where
3 x bvh_depth > 16 the HBM spill area is armed, and in nested and nested_08 (whose rays reach it) it must have been written, as in the
needle room.

Which rays a scene can be judged on is decided without a GPU by tests/test_hard_scenes_cpu.py (the caps on ambiguous rays and misses, and
hard_scenes.UNCAPPED for the scenes whose rays the verdict's own bands swallow); the CPU oracle's figures below are from there.
Each case prints its ambiguous share, worst |dt| / tt and smallest clear margin (pytest -s).

Measured on an MI355X with K = 64, KT = 16 (the CPU oracle on the same rays in brackets, from tests/test_hard_scenes_cpu.py): unexplained
answers 0 on every entry point, scene and family [0] -- after the builder learnt to give a zero-area triangle a record that cannot be hit
(lbvh.cpp: zero_area; before, `duplicates` had 2 unexplained closest-hit and 1 unexplained any-hit answer in `edge` through traverse<>,
the first entry point run: the FP32 determinant of three collinear corners is rounding noise, not zero, and a ray along their line was
answered u = v = 0, t = 2.0).  Worst |dt| / tt among unambiguous hits 0.052 (mixed_scale `outside`, traverse<>) [0.057, the same rays]; per scene at most:
tiny_k 0.029 [0.035], flat 0.011 [0.008], far_64 0.016 [0.017], far_256 0.012 [0.012], far_4096 0.000 [0.000] (tt itself is ~ 0.1
there), far_tiles 0.014 [0.012], far_tiles_256 0.006 [0.006], duplicates 0.041 [0.036], mixed_scale_2000 0.025 [0.027], nested 0.038
[0.039], nested_08 0.027 [0.030].  Smallest clear margin dist|cos| / dw of an accepted unambiguous hit 1.00 [1.00] -- the definition's
floor -- in every group of scenes.  The ambiguous shares are the inputs' (the table of tests/test_hard_scenes_cpu.py).  nested:
3 x bvh_depth = 27, nested_08: 57; the HBM spill area is written by traverse<> and by the pooled pass in both; trace_bench modes 2 and 3
refuse nested_08 (57 > 48).  The 160 cases take 6 s together.
"""
import pytest

from tests import hard_scenes as hs
from tests import test_gpu_ray_verdict as base
from tests.test_gpu_ray_verdict import _pattern, _pool_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=hs.HARD_SCENES, ids=[s[0] for s in hs.HARD_SCENES])
def sc(request, gpu, pkg):
    name, kw = request.param
    c = hs.build_scene_cases(pkg, name, kw)
    r = pkg.Renderer(c["scene"], 0)
    info = r.scene_info()
    assert info["n_triangles"] == c["verdict"].T, info
    # deep: the tree has an HBM part of the stack at all; nest: rays are known to reach it (tests/test_hard_scenes_cpu.py: the deepest stack
    # of tools/bvh_eval.cpp's traversal over these very families is 23 entries in nested and 52 in nested_08, against 16 in LDS)
    return dict(c, renderer=r, deep=3 * info["bvh_depth"] - 16 > 0, nest=name.startswith("nested"))


def test_the_deep_scenes_are_deep(sc):
    if sc["name"] in ("nested", "nested_08"):
        assert sc["deep"], sc["renderer"].scene_info()


def test_traverse_answers_are_all_explained(sc):
    r = sc["renderer"]
    if sc["deep"]:
        r.trace_closest(sc["cases"]["random"]["rays"])   # sizes the spill area
        r.spill_arm()
    base.test_traverse_answers_are_all_explained(sc)
    if sc["nest"]:
        assert r.spill_count()[0] > 0, r.spill_count()


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_trace_bench_answers_are_all_explained(sc, pkg, mode):
    """(a mode whose per-ray stack does not hold 3 x bvh_depth entries has to refuse: the rule of the test this calls)"""
    base.test_trace_bench_answers_are_all_explained(sc, pkg, mode)


def test_pooled_pass_answers_are_all_explained(sc):
    r = sc["renderer"]
    if sc["deep"]:
        fam = sc["cases"]["random"]
        r.trace_pool(*_pool_inputs(fam, *_pattern("full", len(fam["rays"]))))   # sizes the spill area
        r.spill_arm()
    base.test_pooled_pass_answers_are_all_explained(sc)
    if sc["nest"]:
        assert r.spill_count()[0] > 0, r.spill_count()


@pytest.mark.parametrize("knob", ["SPCBPT_NO_FAN_TAIL", "SPCBPT_BVH_HOT_NODES"])
def test_pooled_pass_without_fan_tail_and_without_hot_order(sc, pkg, monkeypatch, knob):
    base.test_pooled_pass_without_fan_tail_and_without_hot_order(sc, pkg, monkeypatch, knob)
