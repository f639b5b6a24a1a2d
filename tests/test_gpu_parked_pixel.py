"""The batched eye kernel keeps a parked pixel's radiance in the film of the pixel's frame (csrc/eye_kernel_body.h): a lane whose
path ended at a vertex that still owes its connections stores the radiance so far at once, takes the next pixel-sample, and -- only
if one of the owed connections turns out unoccluded -- reads the value back after the connect phase, adds the contributions in
connection order and stores it again.  The value round-trips through memory bit for bit and no sum changes its order, so a batched launch must
leave the film of frame-by-frame launches (spcbpt_launch per frame: `pend_result` in registers, film_write) exactly, from the same
subframes, the same samplers and one tuple trained on the spot.  The shapes are those at which a parked pixel would go wrong:
  * 16 x 8 pixels, 32 frames in one launch: two tiles per frame, so every wave holds lanes of several frames at once -- parked pixels,
    their vertices and their films belong to different frames within one wave;
  * 70 x 36 pixels, 3 frames: partial tiles on both edges, pool slots outside the image;
  * the small hallway, 64 x 64, 5 frames: long paths, most of which end by Russian roulette with connections still owed.
The film after frame k is the running mean of frames 0..k; the snapshots of the frame-by-frame run must differ from each other
and from zero, so that an empty film cannot pass for agreement."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = {"cornell 16x8, 32 frames": ("cornell", 16, 8, 32, (3000, 64, 1)),
         "cornell 70x36, 3 frames": ("cornell", 70, 36, 3, (3000, 64, 1)),
         "hallway 64x64, 5 frames": ("hallway", 64, 64, 5, (8000, 52, 1))}


def _renderer(pkg, scene, w, h, lt, batch):
    if batch > 1:
        os.environ["SPCBPT_EYE_BATCH"] = str(batch)    # sizes the ring of buffer sets: `batch` samplers stay intact side by side
    try:
        r = pkg.Renderer(scene, 0)
    finally:
        os.environ.pop("SPCBPT_EYE_BATCH", None)
    cam = scene.camera
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
    r.resize(w, h)
    r.set_light_trace(*lt)
    return r


@pytest.mark.parametrize("case", list(CASES))
def test_batched_films_equal_frame_by_frame_launches(gpu, pkg, case):
    name, w, h, frames, lt = CASES[case]
    scene = pkg.scenes.cornell_box() if name == "cornell" else pkg.scenes.hallway(target_tris=4000)
    a = _renderer(pkg, scene, w, h, lt, 1)
    a.set_pretrace(20000, 10)
    a.preprocess(target_paths=100000, target_q_paths=100000, train=True)
    tup = a.get_subspace()
    snaps = []
    for f in range(frames):
        a.launch("light trace", f + 1); a.build_sampler(); a.launch("SPCBPT_eye", f)
        a.sync()
        snaps.append(a.read_accum().copy())
    want = snaps[-1]
    assert np.isfinite(want).all()
    assert all((s[..., :3] != 0).any() for s in snaps), "an empty film"
    assert all(not np.array_equal(snaps[k], snaps[k + 1]) for k in range(frames - 1)), "a frame that changed nothing"
    b = _renderer(pkg, scene, w, h, lt, frames)
    b.set_subspace(*tup)
    for rep in range(2):                     # twice: the film must not depend on which lanes the queue gave the tiles to
        b.clear_accum()
        for f in range(frames):
            b.launch("light trace", f + 1); b.build_sampler()
        b.launch_eye_batch(list(range(frames)))
        b.sync()
        got = b.read_accum()
        assert np.array_equal(got, want), (rep, int((got != want).any(-1).sum()), float(np.abs(got - want).max()))
