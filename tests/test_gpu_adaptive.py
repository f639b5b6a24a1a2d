"""Adaptive sampling on the device (spcbpt_adaptive_*, spcbpt_launch_adaptive): the tile selection against the host form, every
adaptive sample against the uniform renderer's -- byte for byte: a pixel of a tile at sample index s is seeded, weighted and merged as
an ordinary launch of subframe s would, so accum, the RGBA8 frame and the moments plane must EQUAL those of contexts that only ever
launch ordinarily -- the tiles a launch does not list, the state machine, the loop's end and the render tool.

Cornell box, 4 000 light paths, films of 48x32 (6 x 4 whole tiles) and 43x29 (6 x 4 tiles, the last column 3 pixels wide, the last row
5 pixels high).  The library under test is the IEEE build.  Bars: device tile errors within 1e-5 relative of the host's (they run the
same float32 operations in the same order; the bar is tests/test_adaptive_host.py's), lists equal with the target in the middle of a
gap of at least 1e-3 relative between two neighbouring tile errors; everything else exact."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests.test_gpu_mesh_light import _renderer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, STATE = -1, -5
LIGHT = (4000, 16, 1)
SIZES = [(48, 32), (43, 29)]
IDS = ["48x32", "43x29"]


def _fails(pkg, fn, code, text=None):
    with pytest.raises(pkg.SpcbptError) as e:
        fn()
    assert f"({code})" in str(e.value), str(e.value)
    if text:
        assert text in str(e.value), str(e.value)


def _context(pkg, hip_lib, w, h):
    assert hip_lib.spcbpt_build_arithmetic().decode() == "ieee"
    r = _renderer(pkg, pkg.scenes.cornell_box(), w, h, light=LIGHT, tuple_="minimal")
    r.set_film_moments(True)
    return r


def _light(r, launch_frame):
    r.launch("light trace", launch_frame)
    r.build_sampler()


def _uniform(r, subframe, launch_frame=None):
    _light(r, subframe + 1 if launch_frame is None else launch_frame)
    r.launch("SPCBPT_eye", subframe)


def _planes(r):
    return r.read_accum().copy(), r.read_frame().copy(), r.read_film_moments().copy()


def _tile(t, w, h):
    tx = (w + 7) // 8
    x0, y0 = (t % tx) * 8, (t // tx) * 8
    return slice(y0, min(y0 + 8, h)), slice(x0, min(x0 + 8, w))


def _same_tile(a, b, t, w, h):
    ys, xs = _tile(t, w, h)
    return all(p[ys, xs].tobytes() == q[ys, xs].tobytes() for p, q in zip(a, b))


def _gap_target(err):
    e = np.sort(np.asarray(err, np.float64).reshape(-1))
    e = e[e > 0]
    gaps = [(abs(i - e.size // 2), i) for i in range(1, e.size) if e[i] - e[i - 1] >= 1e-3 * e[i]]
    assert gaps, "the film holds no gap of 1e-3 relative between neighbouring tile errors"
    i = min(gaps)[1]
    return 0.5 * (e[i - 1] + e[i])


# ------------------------------------------------------------------------------------------------------------ selection
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_device_selection_equals_host(gpu, pkg, hip_lib, size):
    w, h = size
    r = _context(pkg, hip_lib, w, h)
    _uniform(r, 0)
    one = _planes(r)
    for f in range(1, 8):
        _uniform(r, f)
    accum, _, m2n = _planes(r)
    r.adaptive_begin(8)
    st = r.adaptive_state()
    assert st == {"active": True, "tiles_x": 6, "tiles_y": 4, "n_listed": 0}
    eights = np.full((4, 6), 8, np.uint32)
    host_err = pkg.api.adaptive_select_host(accum, m2n, eights, 0.0)["error"]
    target = _gap_target(host_err)
    for mn, mx in ((0, 0), (4, 64)):
        host = pkg.api.adaptive_select_host(accum, m2n, eights, target, mn, mx)
        n = r.adaptive_select(target, mn, mx)
        a = r.read_adaptive()
        assert r.adaptive_select(target, mn, mx) == n
        b = r.read_adaptive()
        assert all(a[k].tobytes() == b[k].tobytes() for k in ("samples", "error", "tiles"))       # no atomics: the same film, the same bits
        assert n == a["tiles"].size == r.adaptive_state()["n_listed"]
        assert np.all(a["samples"] == 8)
        pos = host["error"] > 0
        assert pos.sum() >= 12 and np.all(a["error"][~pos] == 0)
        rel = np.abs(a["error"][pos].astype(np.float64) / host["error"][pos] - 1).max()
        print(f"{w}x{h}: tile errors {host['error'].min():.4g} .. {host['error'].max():.4g}, device - host {rel:.3g} relative; target {target:.4g}: {n} of 24 tiles")
        assert rel <= 1e-5
        assert a["tiles"].tolist() == host["tiles"].tolist() and 0 < n < 24
        assert np.all(np.diff(a["tiles"].astype(np.int64)) > 0)
    # the floor and the cap: every tile is short of 9 samples; no tile is below a cap of 8
    assert r.adaptive_select(target, 9, 0) == 24 and r.read_adaptive()["tiles"].tolist() == list(range(24))
    assert r.adaptive_select(target, 0, 8) == 0 and r.read_adaptive()["tiles"].size == 0
    assert r.adaptive_select(0.0, 0, 0) == pkg.api.adaptive_select_host(accum, m2n, eights, 0.0)["tiles"].size
    # unknown tiles: a film of ONE frame declared to hold 8 -- no pixel has two samples, every tile is listed whatever the target, the
    # error reads 0; the cap still holds them back
    r.clear_accum()
    assert r.adaptive_state()["active"] is False
    _uniform(r, 0)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(_planes(r), one))
    r.adaptive_begin(8)
    host = pkg.api.adaptive_select_host(one[0], one[2], eights, 1e30)
    assert r.adaptive_select(1e30) == 24 == host["tiles"].size
    a = r.read_adaptive()
    assert not a["error"].any() and not host["error"].any() and a["tiles"].tolist() == list(range(24))
    assert r.adaptive_select(1e30, 0, 8) == 0
    # all-black tiles: with the camera turned away every sample is zero -- e_t = 0 and KNOWN: nothing is above a target of 0, and only
    # the floor of two samples lists them
    cam = pkg.scenes.cornell_box().camera
    U, V, W = pkg.camera_frame(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
    r.set_camera(np.array(cam["eye"], np.float32), U, V, -np.asarray(W, np.float32))
    r.clear_accum()
    _uniform(r, 0)
    _uniform(r, 1)
    black = _planes(r)
    assert not black[0][..., :3].any() and np.all(black[2][..., 3] == 2)
    r.adaptive_begin(2)
    assert r.adaptive_select(0.0) == 0 and not r.read_adaptive()["error"].any()
    assert pkg.api.adaptive_select_host(black[0], black[2], np.full(24, 2, np.uint32), 0.0)["tiles"].size == 0
    assert r.adaptive_select(0.0, 3, 0) == 24


# ------------------------------------------------------------------------------------------------------------ every sample is the uniform renderer's
@pytest.mark.parametrize("size", SIZES, ids=IDS)
def test_adaptive_samples_are_the_uniform_renderers(gpu, pkg, hip_lib, size):
    """A launches ordinarily only.  B renders frames 0..3 ordinarily, then adaptively: all tiles, S, S, then S + T.  C is T's twin: it gives
    every pixel the (light-pass frame, sample index) pairs T's pixels saw in B, through ordinary launches."""
    w, h = size
    S, T = [0, 8, 23], 15            # first tile, an interior tile, the last tile (43x29: the partial corner); T is another interior tile
    rest = [t for t in range(24) if t not in S]
    a_ctx, b_ctx, c_ctx = (_context(pkg, hip_lib, w, h) for _ in range(3))
    A = []
    for f in range(8):
        _uniform(a_ctx, f)
        A.append(_planes(a_ctx))
    for f in range(4):
        _uniform(b_ctx, f)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(_planes(b_ctx), A[3]))
    b_ctx.adaptive_begin(4)
    counts = np.full(24, 4, np.uint32)

    def step(launch_frame, tiles):
        _light(b_ctx, launch_frame)
        b_ctx.adaptive_set_tiles(tiles)
        assert b_ctx.adaptive_state()["n_listed"] == len(tiles)
        b_ctx.launch_adaptive()
        counts[tiles] += 1
        got = b_ctx.read_adaptive()
        assert got["samples"].reshape(-1).tolist() == counts.tolist() and got["tiles"].tolist() == list(tiles)
        planes = _planes(b_ctx)
        for t in range(24):                                                    # the moments plane's n is the tile's count at every pixel
            ys, xs = _tile(t, w, h)
            assert np.all(planes[2][ys, xs, 3] == counts[t])
        return planes

    B = step(5, list(range(24)))                                               # sample 4 under light pass 5, everywhere: A's frame 4
    assert all(p.tobytes() == q.tobytes() for p, q in zip(B, A[4]))
    for f in (5, 6):                                                           # S moves on with A; the others stay where they were
        before = B
        B = step(f + 1, S)
        assert all(_same_tile(B, A[f], t, w, h) for t in S)
        assert all(_same_tile(B, A[4], t, w, h) and _same_tile(B, before, t, w, h) for t in rest)
        assert not _same_tile(B, before, S[1], w, h)
    # the empty list: success, and nothing changes
    _light(b_ctx, 99)
    b_ctx.adaptive_set_tiles([])
    b_ctx.launch_adaptive()
    assert all(p.tobytes() == q.tobytes() for p, q in zip(_planes(b_ctx), B))
    assert b_ctx.read_adaptive()["samples"].reshape(-1).tolist() == counts.tolist()
    # T's sample index (5) now lags the light pass's frame (8): its twin C renders sample 5 under light pass 8 with an ordinary launch
    before = B
    B = step(8, sorted(S + [T]))
    assert all(_same_tile(B, A[7], t, w, h) for t in S)
    for f in range(5):
        _uniform(c_ctx, f)
    _uniform(c_ctx, 5, launch_frame=8)
    Cp = _planes(c_ctx)
    assert _same_tile(B, Cp, T, w, h) and not _same_tile(B, A[5], T, w, h)
    assert all(_same_tile(B, before, t, w, h) for t in rest if t != T)
    # back to ordinary launches: a uniform frame merges everywhere again (subframe 0 restarts the film)
    b_ctx.adaptive_end()
    assert b_ctx.adaptive_state() == {"active": False, "tiles_x": 0, "tiles_y": 0, "n_listed": 0}
    assert all(p.tobytes() == q.tobytes() for p, q in zip(_planes(b_ctx), B))   # the film is left as it is
    _uniform(b_ctx, 0)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(_planes(b_ctx), A[0]))


def test_adaptive_from_an_empty_film(gpu, pkg, hip_lib):
    """adaptive_begin(0): sample 0 of every tile restarts the film exactly as subframe 0 does; a partial list leaves the rest zero."""
    w, h = 43, 29
    a_ctx, b_ctx = _context(pkg, hip_lib, w, h), _context(pkg, hip_lib, w, h)
    _uniform(a_ctx, 0)
    A0 = _planes(a_ctx)
    b_ctx.adaptive_begin(0)
    _light(b_ctx, 1)
    b_ctx.adaptive_set_tiles([5, 23])
    b_ctx.launch_adaptive()
    B = _planes(b_ctx)
    assert _same_tile(B, A0, 5, w, h) and _same_tile(B, A0, 23, w, h)
    assert all(not p[_tile(t, w, h)].any() for p in B for t in range(24) if t not in (5, 23))
    b_ctx.adaptive_set_tiles([t for t in range(24) if t not in (5, 23)])
    b_ctx.launch_adaptive()
    assert all(p.tobytes() == q.tobytes() for p, q in zip(_planes(b_ctx), A0))
    assert np.all(b_ctx.read_adaptive()["samples"] == 1)


# ------------------------------------------------------------------------------------------------------------ state machine
def test_state_machine(gpu, pkg, hip_lib):
    w, h = 43, 29
    scene = pkg.scenes.cornell_box()
    r = _renderer(pkg, scene, w, h, light=LIGHT, tuple_="minimal")
    _fails(pkg, lambda: r.adaptive_begin(0), STATE, "moments")                 # needs the moments
    for fn in (lambda: r.adaptive_select(0.1), r.launch_adaptive, r.read_adaptive, lambda: r.adaptive_set_tiles([0])):
        _fails(pkg, fn, STATE, "not active")
    r.adaptive_end()                                                           # ending what is not active is no error
    r.set_film_moments(True)
    r.launch_deferred("pt", 0)
    _fails(pkg, lambda: r.adaptive_begin(0), STATE, "deferred")
    r.merge_deferred(True)
    _uniform(r, 1)
    r.adaptive_begin(2)
    # launches that merge with one weight for all pixels are refused, by name
    for alg in ("pt", "SPCBPT_eye", "SPCBPT_no_rmis", "lt"):
        _fails(pkg, lambda a=alg: r.launch(a, 2), STATE, "adaptive sampling")
    _fails(pkg, lambda: r.launch_deferred("SPCBPT_eye", 2), STATE, "adaptive sampling")
    _fails(pkg, lambda: r.launch_deferred("pt", 2), STATE, "adaptive sampling")
    _fails(pkg, lambda: r.launch_eye_batch([2]), STATE, "adaptive sampling")
    _fails(pkg, lambda: r.set_film_moments(False), STATE, "adaptive sampling")
    # ... and what only reads the film is not
    before = _planes(r)
    _light(r, 3)
    r.launch_features(0)
    r.denoise_variance(1)
    assert r.film_error()["pixels"] == w * h
    assert all(p.tobytes() == q.tobytes() for p, q in zip(_planes(r), before))
    # the list: strictly ascending and in range
    for bad in ([3, 2], [2, 2], [0, 24], [24], list(range(24)) + [23]):
        _fails(pkg, lambda b=bad: r.adaptive_set_tiles(b), INVALID, "adaptive_set_tiles")
    assert r.adaptive_state()["n_listed"] == 0
    r.adaptive_set_tiles([1, 2, 7])
    _fails(pkg, lambda: r.launch_adaptive("pt"), INVALID, "SPCBPT_eye")
    _fails(pkg, lambda: r.launch_adaptive("lt"), INVALID, "SPCBPT_eye")
    r.enable_counters(True)
    _fails(pkg, r.launch_adaptive, STATE, "counters")
    r.enable_counters(False)
    r.launch_adaptive()
    assert r.read_adaptive()["samples"].reshape(-1).tolist() == [3 if t in (1, 2, 7) else 2 for t in range(24)]
    # resize and clear_accum end the mode; after adaptive_end an ordinary launch works again
    r.clear_accum()
    assert r.adaptive_state()["active"] is False
    _fails(pkg, r.launch_adaptive, STATE, "not active")
    _uniform(r, 0)
    r.adaptive_begin(1)
    r.resize(w, h)
    assert r.adaptive_state()["active"] is False and r.film_moments()
    _uniform(r, 0)
    r.adaptive_begin(1)
    r.adaptive_end()
    _uniform(r, 1)
    assert np.all(r.read_film_moments()[..., 3] == 2)
    # without a sampler the launch is refused like spcbpt_launch("SPCBPT_eye")
    q = _renderer(pkg, scene, w, h, light=LIGHT)
    q.set_film_moments(True)
    q.adaptive_begin(0)
    q.adaptive_set_tiles([0])
    _fails(pkg, q.launch_adaptive, STATE, "sampler")


def test_sky_seeing_mode_is_refused(gpu, pkg, hip_lib):
    w, h = 48, 32
    r = _renderer(pkg, pkg.scenes.cornell_box(), w, h, light=LIGHT)
    sky = np.ones((8, 16, 4), np.float32)
    r.set_environment(sky)
    r.set_subspace()
    r.set_film_moments(True)
    _uniform(r, 0)
    r.adaptive_begin(1)
    r.adaptive_set_tiles([0, 23])
    r.set_environment_mode(pkg.api.ENV_EYE_SEES_SKY)
    _fails(pkg, r.launch_adaptive, STATE, "sky")
    r.set_environment_mode(0)
    _light(r, 2)
    r.launch_adaptive()                                                        # the general (ENV) instantiation
    n = r.read_film_moments()[..., 3]
    assert np.all(n[:8, :8] == 2) and np.all(n[24:, 40:] == 2) and np.all(n[8:24] == 1)
    assert np.isfinite(r.read_accum()).all()


# ------------------------------------------------------------------------------------------------------------ the loop
def test_loop_ends_where_it_says(gpu, pkg, hip_lib):
    w, h = 48, 32
    mn, mx = 4, 64
    r = _context(pkg, hip_lib, w, h)
    for f in range(8):
        _uniform(r, f)
    r.adaptive_begin(8)
    r.adaptive_select(0.0)
    target = float(np.median(r.read_adaptive()["error"]))                      # from the film itself: about half the tiles start below it
    assert target > 0
    r.clear_accum()
    for f in range(mn):
        _uniform(r, f)
    r.adaptive_begin(mn)
    launched, rounds = 0, 0
    while True:
        n = r.adaptive_select(target, mn, mx)
        if n == 0:
            break
        rounds += 1
        assert rounds <= mx - mn, "the selection never emptied"
        _light(r, 100 + rounds)
        r.launch_adaptive()
        launched += n
    state = r.read_adaptive()
    samples = state["samples"].reshape(-1)
    accum, _, m2n = _planes(r)
    host = pkg.api.adaptive_select_host(accum, m2n, samples, target, mn, mx)
    err = host["error"].reshape(-1)
    assert host["tiles"].size == 0                                              # no tile is selectable any more ...
    assert np.all((samples == mx) | ((samples >= mn) & (err <= target)))       # ... each for one of the two reasons
    assert int(samples.sum()) == 24 * mn + launched
    for t in range(24):
        ys, xs = _tile(t, w, h)
        assert np.all(m2n[ys, xs, 3] == samples[t])
    print(f"48x32, target {target:.4g} (median tile error at 8 frames): {rounds} rounds, tile-samples used {int(samples.sum())} against "
          f"tiles x max count = 24 x {int(samples.max())} = {24 * int(samples.max())}; counts {int(samples.min())} .. {int(samples.max())}, "
          f"{int((samples == mx).sum())} tiles at the cap")
    assert samples.max() > samples.min()


# ------------------------------------------------------------------------------------------------------------ the tool
def test_render_tool_adaptive(gpu, pkg, tmp_path):
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "spcbpt_render"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    data = os.path.join(ROOT, "scenes", "data")
    out = os.path.join(str(tmp_path), "tool")
    cmd = [os.path.join(ROOT, "tools", "spcbpt_render"), os.path.join(data, "cornell", "cornell.scene"), data, "--alg", "SPCBPT_eye", "--minimal", "--dim=64x40",
           "--frames", "24", "--adaptive", "--target-error", "0.05", "--min-samples", "4", "--out", out]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:]
    m = re.search(r"adaptive: target error 0.05, 4 uniform frames, (\d+) rounds, (\d+) adaptive launches; tile-samples traced (\d+) of (\d+) \(tiles x frames = 40 x 24\)", p.stdout)
    assert m, p.stdout[-3000:]
    rounds, launches, traced, full = (int(v) for v in m.groups())
    print(p.stdout[p.stdout.index("adaptive:"):].strip())
    assert full == 40 * 24 and 40 * 4 <= traced <= full and launches == rounds <= 20
    head, body = open(out + "_samples.pgm", "rb").read().split(b"\n", 3)[:3], open(out + "_samples.pgm", "rb").read().split(b"\n", 3)[3]
    assert head[0] == b"P5" and head[1] == b"8 5" and 4 <= int(head[2]) <= 24 and len(body) == 40
    assert sum(body) == traced and max(body) == int(head[2]) and min(body) >= 4
    assert os.path.getsize(out + ".pfm") > 64 * 40 * 12 and os.path.getsize(out + ".ppm") > 64 * 40 * 3
