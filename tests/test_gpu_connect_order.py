"""The connect phase lists its jobs by kind (csrc/job_order.h: connections to surface light vertices first, connections to vertices
on an emitter after them, each group in (connection, lane) order), so that whole rounds of 64 jobs run one arm of connect_vertices.  That
is scheduling: no film may change by a bit.  Two small scenes, SPCBPT_eye with the minimal tuple, set_light_trace(2000, 64, 1), two
subframes:
  * cornell_box() at 32 x 32 -- waves reach more than 128 jobs and see the lit ceiling: emitter hits and jobs of both kinds;
  * scenes.needle_room(4000) at 48 x 32 -- waves with few jobs or none.
Three ways to run each:
  * "plain"    -- the kind bit of a job is right;
  * "uniform"  -- set_connection_sampler(1): the uniform comparator draws no light subspace, every bit is 0;
  * "mirrored" -- every light pass's cache goes through lvc_read / lvc_import with subspace_id replaced by 999 - subspace_id, so the
                  bit (taken from the subspace the first stage drew) is wrong for the emitter patches' labels and for as many
                  surface labels: connect_vertices still branches on the vertex's depth, so only the order of the jobs changes.
For each: the film hashes (tools/film_dump.py's hashing) to what the build of the commit BEFORE the change rendered for the same
calls (tests/golden/connect_order_hashes.json), a 2-frame batched launch equals two single launches bit for bit, and sync()
raises nothing."""
import importlib.util
import json
import os

import numpy as np
import pytest

from tests.parity_util import minimal_tuple

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = {"cornell": (lambda pkg: pkg.scenes.cornell_box(), 32, 32),
          "needles": (lambda pkg: pkg.scenes.needle_room(4000), 48, 32)}
MODES = ("plain", "uniform", "mirrored")
NF = 2
_setup = {}   # scene name -> (scene, tuple): the oracle trains the minimal tuple once per scene


def scene_and_tuple(pkg, ob, name):
    if name not in _setup:
        make, W, H = SCENES[name]
        scene = make(pkg)
        cam = scene.camera
        o = ob.Oracle(scene)
        o.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
        o.resize(W, H)
        o.set_light_trace(2000, 64, 1)
        _setup[name] = (scene, minimal_tuple(o, 2))
    return _setup[name]


def render(pkg, ob, name, mode):
    """{"single": film of two single launches, "batched": film of one 2-frame launch} of one scene in one mode."""
    _, W, H = SCENES[name]
    scene, tup = scene_and_tuple(pkg, ob, name)
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
        r.set_subspace(*tup)
        if mode == "uniform":
            r.set_connection_sampler(1)
        return r

    def light_pass_and_sampler(r, f):
        r.launch("light trace", f + 1)
        if mode == "mirrored":
            lvc = r.lvc_read()
            lvc["subspace_id"] = 999 - lvc["subspace_id"]
            r.lvc_import(lvc)
        r.build_sampler()

    a = renderer(1)
    for f in range(NF):
        light_pass_and_sampler(a, f)
        a.launch("SPCBPT_eye", f)
    a.sync()
    single = a.read_accum().copy()
    b = renderer(NF)
    for f in range(NF):
        light_pass_and_sampler(b, f)
    b.launch_eye_batch(list(range(NF)))
    b.sync()
    return {"single": single, "batched": b.read_accum().copy()}


def film_hash(film):
    spec = importlib.util.spec_from_file_location("film_dump", os.path.join(ROOT, "tools", "film_dump.py"))
    fd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fd)
    return fd.hashes({"film": film})["film"]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SCENES))
def test_film_is_the_parent_s_whatever_the_job_order(gpu, pkg, ob, name, mode):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "connect_order_hashes.json")))["films"][name][mode]
    got = render(pkg, ob, name, mode)
    print(name, mode, "hash", film_hash(got["single"]))
    assert np.isfinite(got["single"]).all() and got["single"][..., :3].sum() > 0
    assert np.array_equal(got["batched"], got["single"])
    assert film_hash(got["single"]) == want, "film changed against the build before the jobs were listed by kind"
