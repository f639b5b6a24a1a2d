"""The pooled traversal step without control flow around its stack bookkeeping (csrc/dev_traversal.h: SPC_NODE_STEP_FLAT_Q, the
node step of the LDS-only instantiation of trace_pool, with a sort that carries the child words) must not change a film by a bit.  Two small scenes, SPCBPT_eye with the minimal tuple,
two subframes:
  * scenes.needle_room(4000) at 48 x 32 -- room-spanning slivers: stacks run past 13 entries, so the wave's vote alternates between
    the straight-line step and the plain one with the HBM part within a pass;
  * cornell_box() at 32 x 32 -- the stack never leaves the straight-line step.
For each: the film hashes (tools/film_dump.py's hashing) to what the build of the commit BEFORE the change rendered
(tests/golden/needle_film_hash.json), a 2-frame batched launch equals two single launches bit for bit, and sync() reports no stack
overflow (it raises on one)."""
import importlib.util
import json
import os

import numpy as np
import pytest

from tests.parity_util import minimal_tuple

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"needles": (lambda pkg: pkg.scenes.needle_room(4000), 48, 32),
         "cornell": (lambda pkg: pkg.scenes.cornell_box(), 32, 32)}
NF = 2


def render(pkg, ob, name):
    """{"single": film of two single launches, "batched": film of one 2-frame launch, "spill_words": HBM stack words the batched
    launch wrote} of one case."""
    make, W, H = CASES[name]
    scene = make(pkg)
    cam = scene.camera

    def renderer(batch):
        if batch > 1:
            os.environ["SPCBPT_EYE_BATCH"] = str(batch)
        try:
            r = pkg.Renderer(scene, 0)
        finally:
            os.environ.pop("SPCBPT_EYE_BATCH", None)
        r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
        r.resize(W, H)
        r.set_light_trace(2000, 64, 1)
        return r

    o = ob.Oracle(scene)
    o.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
    o.resize(W, H)
    o.set_light_trace(2000, 64, 1)
    tup = minimal_tuple(o, 2)
    a = renderer(1)
    a.set_subspace(*tup)
    for f in range(NF):
        a.launch("light trace", f + 1); a.build_sampler(); a.launch("SPCBPT_eye", f)
    a.sync()                                   # raises on a traversal stack overflow
    single = a.read_accum().copy()
    b = renderer(NF)
    b.set_subspace(*tup)
    for f in range(NF):
        b.launch("light trace", f + 1); b.build_sampler()
    b.launch_eye_batch([0])                    # sizes the stream's spill area, so that its use can be counted below
    b.sync(); b.clear_accum()
    for f in range(NF):
        b.launch("light trace", f + 1); b.build_sampler()
    b.spill_arm()
    b.launch_eye_batch(list(range(NF)))
    b.sync()
    return {"single": single, "batched": b.read_accum().copy(), "spill_words": b.spill_count()[0]}


def film_hash(film):
    spec = importlib.util.spec_from_file_location("film_dump", os.path.join(ROOT, "tools", "film_dump.py"))
    fd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fd)
    return fd.hashes({"film": film})["film"]


@pytest.mark.parametrize("name", list(CASES))
def test_film_of_the_flat_step_is_the_parent_s(gpu, pkg, ob, name):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "needle_film_hash.json")))["films"][name]
    got = render(pkg, ob, name)
    print(name, "spill words", got["spill_words"], "hash", film_hash(got["single"]))
    assert np.isfinite(got["single"]).all() and got["single"][..., :3].sum() > 0
    assert np.array_equal(got["batched"], got["single"])
    if name == "needles":
        assert got["spill_words"] > 0       # stacks did run past the LDS part: both instantiations of the step were in use
    else:
        assert got["spill_words"] == 0
    assert film_hash(got["single"]) == want, "film changed against the build before the flat step"
