"""spcbpt_launch_eye_batch_film: the batched eye launch whose merge keeps the film's second moment and fills its buckets
(csrc/kernels_merge_stats.hip: k_film_merge_batch_stats).  Two contexts on one scene and the same light launch frames: A launches
frame by frame (moments update, bucket update, merge: three kernels per frame), B builds a sampler per frame and launches the eye
kernel and ONE merge per group.  Everything the film carries must be equal byte for byte: accum, the tone-mapped frame, the moment
plane, the bucket planes, the film error and the robust image.  The Cornell box at 48 x 32 (and 44 x 28 for partial tiles and a
rank's bands) with the minimal subspace tuple."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 48, 32
LIGHT0 = 100   # launch frame of subframe 0's light pass; subframe f of a film takes LIGHT0 + (its position in the test's frame sequence)


def _renderer(pkg, w=W, h=H, batch=None):
    scene = pkg.scenes.cornell_box()
    cam = scene.camera
    if batch:
        os.environ["SPCBPT_EYE_BATCH"] = str(batch)   # sizes the ring of sampler buffer sets (read by spcbpt_create)
    try:
        r = pkg.Renderer(scene, 0)
    finally:
        os.environ.pop("SPCBPT_EYE_BATCH", None)
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
    r.resize(w, h)
    r.set_light_trace(3000, 64, 1)
    r.set_subspace()
    return r


def _per_frame(r, subframes, first_light, rows=None):
    for k, sf in enumerate(subframes):
        r.render_frame("SPCBPT_eye", sf, launch_frame=first_light + k, rows=rows)


def _batched(r, subframes, first_light, groups, rows=None):
    """`subframes` in groups of the given sizes: a light pass and a sampler build per frame, one launch_eye_batch_film per group."""
    assert sum(groups) == len(subframes)
    k = 0
    for g in groups:
        for j in range(g):
            r.launch("light trace", first_light + k + j)
            r.build_sampler()
        r.launch_eye_batch_film(subframes[k:k + g], rows)
        k += g


def _state(r, moments, buckets):
    r.sync()
    s = {"accum": r.read_accum().copy(), "frame": r.read_frame().copy()}
    if moments:
        s["m2n"] = r.read_film_moments().copy()
        s["error"] = r.film_error()
    if buckets:
        s["buckets"] = r.read_film_buckets().copy()
        r.robust_resolve(2.0)
        s["robust"], s["robust8"] = (a.copy() for a in r.read_robust())
    return s


def _assert_same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        if key == "error":
            assert a[key] == b[key], (a[key], b[key])
        else:
            assert a[key].tobytes() == b[key].tobytes(), (key, int((a[key] != b[key]).sum()))


def _pair(pkg, moments, buckets, w=W, h=H, batch=8):
    a, b = _renderer(pkg, w, h), _renderer(pkg, w, h, batch=batch)
    for r in (a, b):
        r.set_film_moments(moments)
        r.set_film_buckets(buckets)
    return a, b


def test_moments_only(gpu, pkg):
    a, b = _pair(pkg, True, 0)
    sf = list(range(7))
    _per_frame(a, sf, LIGHT0)
    _batched(b, sf, LIGHT0, [4, 3])
    sa, sb = _state(a, True, 0), _state(b, True, 0)
    _assert_same(sa, sb)
    assert (sb["m2n"][..., 3] == 7).all() and sb["m2n"][..., :3].max() > 0 and sb["error"]["pixels"] == W * H


def test_buckets_only_revisited_inside_and_across_batches(gpu, pkg):
    a, b = _pair(pkg, False, 3)
    sf = list(range(8))
    _per_frame(a, sf, LIGHT0)
    _batched(b, sf, LIGHT0, [5, 3])
    sa, sb = _state(a, False, 3), _state(b, False, 3)
    _assert_same(sa, sb)
    assert sorted(sb["buckets"][:, 0, 0, 3].tolist()) == [2.0, 3.0, 3.0]


def test_both_with_a_list_that_restarts(gpu, pkg):
    a, b = _pair(pkg, True, 7)
    first = list(range(10))
    _per_frame(a, first, LIGHT0)
    _batched(b, first, LIGHT0, [6, 4])
    _assert_same(_state(a, True, 7), _state(b, True, 7))
    tail = [10, 11, 0, 1]
    _per_frame(a, tail, LIGHT0 + 10)
    _batched(b, tail, LIGHT0 + 10, [4])
    sa, sb = _state(a, True, 7), _state(b, True, 7)
    _assert_same(sa, sb)
    assert (sb["m2n"][..., 3] == 2).all()
    assert (sb["buckets"][:2, ..., 3] == 1).all() and (sb["buckets"][2:] == 0).all()


def test_partial_tiles_and_a_ranks_bands(gpu, pkg):
    w, h = 44, 28
    rows = (8, h, 3)   # bands 1, 4, ...: rows 8 .. 15 of this image
    a, b = _pair(pkg, True, 7, w, h)
    _per_frame(a, [0, 1], LIGHT0)
    _batched(b, [0, 1], LIGHT0, [2])
    before = _state(b, True, 7)
    _assert_same(_state(a, True, 7), before)
    sf = [2, 3, 4, 5, 6]
    _per_frame(a, sf, LIGHT0 + 2, rows)
    _batched(b, sf, LIGHT0 + 2, [3, 2], rows)
    sa, sb = _state(a, True, 7), _state(b, True, 7)
    _assert_same(sa, sb)
    inside = np.zeros(h, bool)
    inside[8:16] = True
    for key in ("accum", "frame", "m2n"):
        assert (sb[key][~inside] == before[key][~inside]).all(), key
        assert (sb[key][inside] != before[key][inside]).any(), key
    assert (sb["buckets"][:, ~inside] == before["buckets"][:, ~inside]).all()
    assert (sb["m2n"][inside][..., 3] == 7).all() and (sb["m2n"][~inside][..., 3] == 2).all()


def test_one_batch_of_32_frames_and_32_buckets(gpu, pkg):
    a, b = _pair(pkg, True, 32, batch=32)
    sf = list(range(32))
    _per_frame(a, sf, LIGHT0)
    _batched(b, sf, LIGHT0, [32])
    sa, sb = _state(a, True, 32), _state(b, True, 32)
    _assert_same(sa, sb)
    assert (sb["buckets"][..., 3] == 1).all()


def test_moments_switched_on_in_mid_film(gpu, pkg):
    a, b = _pair(pkg, False, 0)
    _per_frame(a, [0, 1, 2], LIGHT0)
    _batched(b, [0, 1, 2], LIGHT0, [3])
    for r in (a, b):
        r.set_film_moments(True)
    sf = [3, 4, 5, 6]
    _per_frame(a, sf, LIGHT0 + 3)
    _batched(b, sf, LIGHT0 + 3, [4])
    sa, sb = _state(a, True, 0), _state(b, True, 0)
    _assert_same(sa, sb)
    assert (sb["m2n"][..., 3] == 4).all()


def test_with_both_switches_off_it_is_launch_eye_batch(gpu, pkg):
    a, b = _renderer(pkg, batch=8), _renderer(pkg, batch=8)
    for k in range(5):
        for r in (a, b):
            r.launch("light trace", LIGHT0 + k)
            r.build_sampler()
    a.launch_eye_batch(list(range(5)))
    b.launch_eye_batch_film(list(range(5)))
    _assert_same(_state(a, False, 0), _state(b, False, 0))


def test_adaptive_sampling_starts_from_the_same_film(gpu, pkg):
    a, b = _pair(pkg, True, 0)
    sf = list(range(6))
    _per_frame(a, sf, LIGHT0)
    _batched(b, sf, LIGHT0, [4, 2])
    got = []
    for r in (a, b):
        r.adaptive_begin(6)
        err = r.film_error()["mean"]
        n = r.adaptive_select(err, 0, 64)   # the film's own mean error as the target: some tiles are above it, some below
        st = r.read_adaptive()
        got.append((n, st["tiles"].tobytes(), st["error"].tobytes(), st["samples"].tobytes()))
    assert got[0] == got[1]
    assert 0 < got[0][0] < (W // 8) * (H // 8)


def _refused(pkg, fn, text):
    with pytest.raises(pkg.SpcbptError) as e:
        fn()
    assert text in str(e.value), str(e.value)


def test_refusals_name_their_reason(gpu, pkg):
    r = _renderer(pkg, batch=4)
    r.set_film_moments(True)
    for k in range(2):
        r.launch("light trace", LIGHT0 + k)
        r.build_sampler()
    _refused(pkg, lambda: r.launch_eye_batch_film([]), "launch_eye_batch_film: 1..32 frames")
    _refused(pkg, lambda: r.launch_eye_batch_film(list(range(33))), "launch_eye_batch_film: 1..32 frames")
    r.set_lens(0.05, 1.0)
    _refused(pkg, lambda: r.launch_eye_batch_film([0, 1]), "no lens form")
    r.set_lens(0.0, 1.0)
    r.enable_counters(True)
    _refused(pkg, lambda: r.launch_eye_batch_film([0, 1]), "event counters")
    r.enable_counters(False)
    # launch_eye_batch itself still refuses with either switch on, in its own words
    _refused(pkg, lambda: r.launch_eye_batch([0, 1]), "keeps no second moment")
    r.set_film_buckets(5)
    r.set_film_moments(False)
    _refused(pkg, lambda: r.launch_eye_batch([0, 1]), "fills no buckets")
    r.set_film_buckets(0)
    r.set_film_moments(True)
    for k in range(2):
        r.launch("light trace", LIGHT0 + k)
        r.build_sampler()
    r.launch_eye_batch_film([0, 1])          # ... and nothing of the above has left the context unable to render
    r.launch("light trace", LIGHT0 + 2)
    r.build_sampler()
    r.launch_deferred("SPCBPT_eye", 2)
    _refused(pkg, lambda: r.launch_eye_batch_film([2]), "deferred frame is outstanding")
    r.merge_deferred(True)
    r.adaptive_begin(3)
    r.launch("light trace", LIGHT0 + 3)
    r.build_sampler()
    _refused(pkg, lambda: r.launch_eye_batch_film([3]), "launch_eye_batch_film: adaptive sampling is active")
    r.adaptive_end()
    r.launch_eye_batch_film([3])
    r.sync()
    assert (r.read_film_moments()[..., 3] == 4).all()


def test_device_planes_equal_the_host_form_on_the_frames_own_samples(gpu, pkg):
    """B's moment and bucket planes against spcbpt_film_merge_batch_host on the frames' samples.  The samples come from A, frame by
    frame, as single-sample films: with 32 buckets a film of n <= 32 frames from subframe 0 holds frame f's sample alone in bucket f
    (n = 1, a = 1: mean = 0 + 1 (x - 0) = x, exactly) -- the sample of subframe f, whose seeds depend on f, which a launch of
    every frame as subframe 0 on a cleared film would not give."""
    n = 9
    a = _renderer(pkg)
    a.set_film_buckets(32)
    _per_frame(a, list(range(n)), LIGHT0)
    a.sync()
    planes_a = a.read_film_buckets()
    assert (planes_a[:n, ..., 3] == 1).all()
    x = planes_a[:n].copy()
    assert x[..., :3].max() > 0
    b = _renderer(pkg, batch=8)
    b.set_film_moments(True)
    b.set_film_buckets(4)
    groups = [5, 4]
    _batched(b, list(range(n)), LIGHT0, groups)
    sb = _state(b, True, 4)
    accum = np.zeros((H, W, 4), np.float32)
    m2n = np.zeros((H, W, 4), np.float32)
    planes = np.zeros((4, H, W, 4), np.float32)
    k = 0
    for g in groups:   # the host call gets the subframes B used, batch by batch
        pkg.api.film_merge_batch_host(x[k:k + g], list(range(k, k + g)), accum, m2n, planes)
        k += g
    assert accum.tobytes() == sb["accum"].tobytes()
    assert m2n.tobytes() == sb["m2n"].tobytes()
    assert planes.tobytes() == sb["buckets"].tobytes()
