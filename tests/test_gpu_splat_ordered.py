"""The ordered mode of the light-tracing estimator "lt" (spcbpt_set_splat_order(ctx, SPCBPT_SPLAT_ORDERED)): every cache vertex's
contribution stored as a record, every pixel the sum of its records in ascending cache order -- so the film is the same BITS on every
run, which the atomic mode (tests/test_gpu_splat.py) cannot promise.  The Cornell box, 2000 light paths, the minimal tuple: the shape
of test_gpu_splat.py's `box`.

Measured on the MI355X: 5 413 vertices give 4 495 records; longest segment 424 (48 x 32, 501 lit pixels), 268 (43 x 29), 1 101 (8 x 8),
4 495 (1 x 1); against the atomic film the largest relative difference is 9.1e-7 under a bar of 5.1e-5, 92 % of the values bit-equal."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_gpu_mesh_light import _renderer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIGHT = (2000, 16, 1)
STATE, INVALID, CAPACITY = -5, -1, -6


def _ordered(pkg, w, h):
    r = _renderer(pkg, pkg.scenes.cornell_box(), w, h, light=LIGHT, tuple_="minimal")
    r.set_splat_order(pkg.api.SPLAT_ORDERED)
    return r


def _film(r):
    r.sync()
    return r.read_accum().copy()


def _frame(pkg, w, h):
    """One ordered "lt" frame as subframe 0 (light pass of launch frame 1) -> renderer, film, cache, records, their host sum."""
    r = _ordered(pkg, w, h)
    r.render_frame("lt", 0)
    film = _film(r)
    v = r.lvc_read()
    rgb, pixel = r.read_splat_records()
    return dict(r=r, w=w, h=h, film=film, lvc=v, rgb=rgb, pixel=pixel, host=pkg.api.splat_sum_host(rgb, pixel, w, h))


def _k_max(pixel):
    return int(np.bincount(pixel[pixel >= 0]).max())


@pytest.fixture(scope="module")
def box(gpu, pkg):
    return _frame(pkg, 48, 32)


@pytest.fixture(scope="module")
def full(box):
    """One full launch of the box's cache on a cleared film (what the band and mode tests compare with)."""
    r = box["r"]
    r.clear_accum()
    cleared = r.read_accum().copy()
    r.launch("lt", 0)
    return dict(cleared=cleared, film=_film(r))


# ------------------------------------------------------------------------------------------------------------ 1, 2
@pytest.mark.parametrize("size", [(48, 32), (43, 29)], ids=["48x32", "43x29"])
def test_the_film_is_the_records_ordered_sum(gpu, pkg, box, size):
    """accum.rgb == splat_sum_host(read_splat_records()) bit for bit, one record slot per cache vertex; 43 x 29 has partial tiles."""
    c = box if size == (48, 32) else _frame(pkg, *size)
    w, h = size
    lit = (c["film"][..., :3] > 0).any(-1)
    print(f"{w}x{h}: {len(c['lvc'])} vertices, {int((c['pixel'] >= 0).sum())} records, {int(lit.sum())} lit pixels, largest segment {_k_max(c['pixel'])}")
    assert len(c["pixel"]) == len(c["rgb"]) == len(c["lvc"]) > 1000
    assert lit.sum() > 300
    assert ((c["pixel"] >= -1) & (c["pixel"] < w * h)).all()
    assert np.isfinite(c["film"]).all() and (c["rgb"][c["pixel"] < 0] == 0).all()
    assert c["film"][..., :3].tobytes() == c["host"].tobytes()
    assert (c["film"][..., 3] == 1).all()


@pytest.mark.parametrize("size", [(8, 8), (1, 1)], ids=["8x8", "1x1"])
def test_long_segments(gpu, pkg, size):
    """Small films, where a pixel receives hundreds (8 x 8) to thousands (1 x 1, the smallest film there is) of records."""
    w, h = size
    c = _frame(pkg, w, h)
    k = _k_max(c["pixel"])
    print(f"{w}x{h}: {int((c['pixel'] >= 0).sum())} records of {len(c['lvc'])} vertices, largest segment {k}")
    assert k > (1000 if size == (1, 1) else 100)
    assert len(c["pixel"]) == len(c["lvc"])
    assert c["film"][..., :3].tobytes() == c["host"].tobytes()


# ------------------------------------------------------------------------------------------------------------ 3
def test_against_the_atomic_mode(gpu, pkg, box, full):
    """The same cache in the atomic mode: the two films differ in the order of k non-negative float32 additions per pixel, each order
    within k 2^-24 of the exact sum, so within 2 k_max 2^-24 of each other (1e-5 where that is smaller: test_band_sets' bar between
    two atomic launches).  No pixel is left out, and the zero pixels coincide."""
    r = box["r"]
    k_max = _k_max(box["pixel"])
    rtol = max(1e-5, 2 * k_max * 2.0 ** -24)
    r.set_splat_order(pkg.api.SPLAT_ATOMIC)
    r.clear_accum()
    r.launch("lt", 0)
    atomic = _film(r)
    r.set_splat_order(pkg.api.SPLAT_ORDERED)
    a, o = atomic[..., :3], full["film"][..., :3]
    dev = (np.abs(a.astype(np.float64) - o) / np.where(o > 0, o, 1.0)).max()
    print(f"largest segment {k_max}: bar {rtol:.3g}, largest relative difference {dev:.3g}; bits equal in {float((a == o).mean()):.4f} of the values")
    assert ((a == 0) == (o == 0)).all()
    assert np.allclose(a, o, rtol=rtol, atol=0.0)
    assert full["film"][..., :3].tobytes() == box["film"][..., :3].tobytes()      # the fixture's own launch, for the record


# ------------------------------------------------------------------------------------------------------------ 4
def test_reproducible(gpu, pkg, box, full):
    """Three launches on one cache, then a fresh context with the same scene and light-pass frame: the same bytes."""
    r = box["r"]
    for k in range(3):
        r.clear_accum()
        r.launch("lt", 0)
        assert _film(r).tobytes() == full["film"].tobytes(), k
    other = _frame(pkg, box["w"], box["h"])
    assert other["lvc"].tobytes() == box["lvc"].tobytes()
    assert other["film"].tobytes() == box["film"].tobytes()
    assert other["pixel"].tobytes() == box["pixel"].tobytes() and other["rgb"].tobytes() == box["rgb"].tobytes()


# ------------------------------------------------------------------------------------------------------------ 5
def test_band_sets(gpu, box, full):
    """Rows (0, 16, 1) then (16, 32, 1) on a cleared film: byte-identical to one full launch; (0, 32, 2) writes bands 0 and 2 only."""
    r, cleared, want = box["r"], full["cleared"], full["film"]
    r.clear_accum()
    r.launch("lt", 0, (0, 16, 1))
    a = _film(r)
    assert a[16:].tobytes() == cleared[16:].tobytes()
    assert a[:16, :, :3].sum() > 0
    _, pixel = r.read_splat_records()
    assert len(pixel) == len(box["pixel"]) and (pixel < 16 * box["w"]).all()      # a record outside the launch's rows is no record
    r.launch("lt", 0, (16, 32, 1))
    b = _film(r)
    assert b.tobytes() == want.tobytes()
    r.clear_accum()
    r.launch("lt", 0, (0, 32, 2))
    c = _film(r)
    for band in (1, 3):
        assert c[8 * band:8 * band + 8].tobytes() == cleared[8 * band:8 * band + 8].tobytes()
    for band in (0, 2):
        rows = slice(8 * band, 8 * band + 8)
        assert c[rows].tobytes() == want[rows].tobytes() and c[rows, :, :3].sum() > 0
    r.clear_accum()


# ------------------------------------------------------------------------------------------------------------ 6
def test_nothing_to_add(gpu, pkg, box):
    """The camera turned away from the scene: every record is -1 and the film exactly 0.  A cache capacity well above the vertex count:
    the padding reaches no pixel -- the film is the default-capacity context's, byte for byte, whether the launch knows the count
    (after a sync the light pass has left it in pinned memory) or runs over the whole capacity."""
    w, h = box["w"], box["h"]
    scene = pkg.scenes.cornell_box()
    cam = scene.camera
    r = _ordered(pkg, w, h)
    U, V, W = pkg.camera_frame(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
    r.set_camera(np.array(cam["eye"], np.float32), U, V, -np.asarray(W, np.float32))
    r.render_frame("lt", 0)
    film = _film(r)
    rgb, pixel = r.read_splat_records()
    assert len(pixel) == len(box["lvc"]) and (pixel == -1).all() and (rgb == 0).all()
    assert film[..., :3].tobytes() == np.zeros((h, w, 3), np.float32).tobytes()
    big = _renderer(pkg, scene, w, h, light=LIGHT, tuple_="minimal")
    big.set_splat_order(1)
    big.lvc_set_capacity(4 * len(box["lvc"]) + 1000)
    big.render_frame("lt", 0)                      # no host wait since the light pass: the launch may run over the whole capacity
    first = _film(big)
    assert big.lvc_capacity()[0] >= 4 * len(box["lvc"])
    assert big.lvc_read().tobytes() == box["lvc"].tobytes()
    assert first.tobytes() == box["film"].tobytes()
    _, pixel = big.read_splat_records()
    assert pixel.tobytes() == box["pixel"].tobytes()
    big.clear_accum()
    big.launch("lt", 0)                            # ... and now the light pass is over
    assert _film(big).tobytes() == box["film"].tobytes()


# ------------------------------------------------------------------------------------------------------------ 7
def test_accumulation(gpu, pkg):
    """Four ordered frames, subframes 0 .. 3, the film's moments on: n = 4 everywhere and the film is the running mean of the four
    per-frame host sums -- film_write's lerp3 (a + t (b - a), t = 1 / (k + 1)) in np.float32 -- bit for bit."""
    w, h = 48, 32
    r = _ordered(pkg, w, h)
    r.set_film_moments(True)
    f = np.float32
    mean = None
    for k in range(4):
        r.render_frame("lt", k)
        r.sync()
        rgb, pixel = r.read_splat_records()
        s = pkg.api.splat_sum_host(rgb, pixel, w, h)
        if k == 0:
            mean = s
        else:
            t = f(1.0) / f(k + 1)
            mean = (mean + (t * (s - mean).astype(f)).astype(f)).astype(f)
    film = _film(r)
    assert (r.read_film_moments()[..., 3] == 4).all()
    assert (mean > 0).any(-1).sum() > 300
    assert film[..., :3].tobytes() == mean.tobytes()


# ------------------------------------------------------------------------------------------------------------ 8
def test_errors_and_defaults(gpu, pkg, box):
    w, h = box["w"], box["h"]
    scene = pkg.scenes.cornell_box()

    def fails(fn, code, text=None):
        with pytest.raises(pkg.SpcbptError) as e:
            fn()
        assert f"({code})" in str(e.value), str(e.value)
        if text:
            assert text in str(e.value), str(e.value)

    r = _renderer(pkg, scene, w, h, light=LIGHT, tuple_="minimal")
    assert r.splat_order() == pkg.api.SPLAT_ATOMIC == 0 and pkg.api.SPLAT_ORDERED == 1
    for bad in (2, -1, 7):
        fails(lambda: r.set_splat_order(bad), INVALID)
    assert r.splat_order() == 0
    fails(r.read_splat_records, STATE)                              # no ordered launch yet
    r.render_frame("lt", 0)                                         # ... and an atomic one is none
    never_switched = _film(r)
    fails(r.read_splat_records, STATE)
    r.set_splat_order(1)
    assert r.splat_order() == 1
    fails(r.read_splat_records, STATE)
    r.launch_deferred("pt", 0)
    fails(lambda: r.set_splat_order(0), STATE, "deferred")
    r.merge_deferred(False)
    r.clear_accum()
    r.launch("lt", 0)
    assert _film(r).tobytes() == box["film"].tobytes()              # the same cache (launch frame 1) as the box's
    rgb, pixel = r.read_splat_records()
    assert len(pixel) == len(box["lvc"])
    fails(lambda: r.read_splat_records(capacity=len(pixel) - 1), CAPACITY)
    import ctypes as C
    n = C.c_int(-1)
    assert r.lib.spcbpt_read_splat_records(r.h, None, None, 0, C.byref(n)) == CAPACITY and n.value == len(pixel)   # count is still set
    assert r.lib.spcbpt_read_splat_records(r.h, None, None, 0, None) == INVALID
    r.resize(w, h)                                                  # a resize forgets the records
    fails(r.read_splat_records, STATE)
    r.launch("lt", 0)
    assert len(r.read_splat_records()[1]) == len(pixel)
    r.set_splat_order(0)                                            # back to atomic: the records go, the atomic film is back
    fails(r.read_splat_records, STATE)
    r.clear_accum()
    r.launch("lt", 0)
    again = _film(r)
    assert np.allclose(again[..., :3], never_switched[..., :3], rtol=1e-5, atol=0.0)
    assert ((again[..., :3] == 0) == (never_switched[..., :3] == 0)).all()
    # every refusal of "lt" holds in both modes
    for mode in (0, 1):
        e = _renderer(pkg, scene, w, h, light=LIGHT, tuple_="minimal")
        e.set_splat_order(mode)
        fails(lambda: e.launch("lt", 0), STATE, "sampler")          # no built sampler
        e.launch("light trace", 1)
        fails(lambda: e.launch("lt", 0), STATE, "sampler")          # a light pass without a build
        e.set_environment(pkg.scenes.sky_texture())
        e.set_subspace()
        e.launch("light trace", 1)
        e.build_sampler()
        fails(lambda: e.launch("lt", 0), STATE, "environment")
        fails(lambda: e.launch_deferred("lt", 0), -4)               # the deferred form does not learn the name


# ------------------------------------------------------------------------------------------------------------ 9
def test_render_tool_ordered(gpu, pkg, tmp_path):
    """tools/spcbpt_render --alg lt --ordered-splat --frames 2, twice: the two PFMs are byte-identical."""
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "spcbpt_render"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-3000:]
    path = pkg.scenes.write_gltf(pkg.scenes.cornell_sphere_lamp(2, 4), str(tmp_path), "sphere_room")
    raws = []
    for k in range(2):
        out = os.path.join(str(tmp_path), f"tool{k}")
        cmd = [os.path.join(ROOT, "tools", "spcbpt_render"), path, ".", "--alg", "lt", "--ordered-splat", "--emissive", "--dim=64x64", "--frames", "2", "--out", out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:]
        assert "2 subframes of lt at 64x64" in r.stdout and "ordered" in r.stdout, r.stdout
        raws.append(open(out + ".pfm", "rb").read())
    head = raws[0].split(b"\n", 3)
    assert head[0] == b"PF" and head[1] == b"64 64"
    img = np.frombuffer(head[3], np.float32).reshape(64, 64, 3)
    assert np.isfinite(img).all() and img.mean() > 0
    assert raws[0] == raws[1]
