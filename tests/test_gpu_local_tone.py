"""The local tone stage on the device (spcbpt_local_tone, spcbpt_local_tone_image): its float4 plane against the host form
spcbpt_local_tone_host run on the same image -- BIT FOR BIT: only + - x /, compares, int <-> float conversions and bit-pattern moves are
on the path and the library under test is the IEEE build, however the gather is cut over lanes and chunks --, the plane as a display
source, that every other plane keeps its bits, and what is refused.  The host form is held to the float64 definition by
tests/test_local_tone_host.py.

Measured on the MI355X: see DESIGN.md 8l."""
import os
import subprocess

import numpy as np
import pytest

from tests import display_ref
from tests import local_tone_ref as ref
from tests.display_ref import tie_mask
from tests.test_gpu_mesh_light import _renderer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, INVALID = -5, -1
FRAMES = 6
IDS = [ref.shape_id(s) for s in ref.SHAPES]
SOURCES = ("film", "denoised", "robust", "history", "bloom")


def _fails(pkg, fn, code, text=None):
    with pytest.raises(pkg.SpcbptError) as e:
        fn()
    assert f"({code})" in str(e.value), str(e.value)
    if text:
        assert text in str(e.value), str(e.value)


def _planes(r):
    """Every plane a local tone call must leave alone, as bytes (the list of tests/test_gpu_bloom.py, with the bloom and display planes)."""
    den, den8 = r.read_denoised()
    rob, rob8 = r.read_robust()
    hist = r.read_history()
    return dict(accum=r.read_accum().tobytes(), frame=r.read_frame().tobytes(), moments=r.read_film_moments().tobytes(), buckets=r.read_film_buckets().tobytes(),
                denoised=den.tobytes(), denoised8=den8.tobytes(), robust=rob.tobytes(), robust8=rob8.tobytes(),
                resolved=hist["resolved"].tobytes(), resolved8=hist["frame"].tobytes(), bloom=r.read_bloom().tobytes(), display=r.read_display()[0].tobytes())


@pytest.fixture(scope="module")
def plain(gpu, pkg, hip_lib):
    assert hip_lib.spcbpt_build_arithmetic().decode() == "ieee"
    return _renderer(pkg, pkg.scenes.cornell_box(), 48, 32)


# ------------------------------------------------------------------------------------------------------------ images of the caller's
@pytest.mark.parametrize("shape", ref.SHAPES, ids=IDS)
def test_local_tone_image_is_the_host_form_bit_for_bit(pkg, plain, shape):
    """The shapes of tests/local_tone_ref.py: footprints cut by every image edge and node columns with no pixel at all (1 x 1, 7 x 1,
    1 x 7), the image inside one cell whose 127-wide footprint is walked in chunks of rows (s = 64), 646 node columns and a ragged
    last block of the slice kernel (130 x 70, s = 4), more bins than a wave has lanes (NZ = 66) and NZ = 6; blur 0, 1 and 4."""
    r = plain
    w, h = shape[:2]
    img, plants = ref.planted_image(w, h)
    for ps in ref.PARAM_SETS:
        kw = dict(ps, cell=shape[2], range=shape[3])
        r.local_tone_image(img, **kw)
        dev = r.read_local_tone()
        assert dev.shape == img.shape and dev.dtype == np.float32
        assert dev.tobytes() == pkg.api.local_tone_host(img, **kw).tobytes(), (shape, kw)
    r.local_tone_image(img, **kw)                              # the same call twice: the same bytes
    assert r.read_local_tone().tobytes() == dev.tobytes()
    no = ref.no_part_mask(plants, img.shape[:2])
    assert np.array_equal(dev.view(np.uint32)[no], img.view(np.uint32)[no])
    assert r.image_size() == (48, 32)                          # the context's film keeps its size


def test_a_tall_footprint_in_chunks_and_the_unit_slopes(pkg, plain):
    """150 x 140 at s = 64: node columns whose footprint is 127 x 127, walked in eight chunks of 16 rows, beside columns cut by the image
    edge; then compress = detail = 1, which returns the source's bits."""
    r = plain
    img, _ = ref.planted_image(150, 140)
    kw = dict(cell=64, range=0.5, blur=1, compress=0.4, detail=1.2)
    r.local_tone_image(img, **kw)
    assert r.read_local_tone().tobytes() == pkg.api.local_tone_host(img, **kw).tobytes()
    r.local_tone_image(img, cell=8, compress=1.0, detail=1.0)
    assert r.read_local_tone().tobytes() == img.tobytes()


def test_few_active_bins_far_apart_many_and_none(pkg, plain):
    """The gather walks the bins that a chunk of its footprint marks.  An edge image has two groups of them twelve bins apart, a ramp
    under little noise a few neighbours that change from column to column (at s = 64 from chunk to chunk), the seeded image nearly
    all; a black image none.  The host form walks every bin: the same bytes."""
    r = plain
    ramp, _ = ref.planted_image(130, 70)
    ramp[..., :3] = (2.0 ** (np.arange(130)[None, :, None] / 13.0 - 5.0) * (1.0 + 0.1 * (ramp[..., :3] > 1.0))).astype(np.float32)
    black = np.zeros((23, 37, 4), np.float32)
    for img, kw in ((ref.edge_image(), dict(cell=8, blur=1)), (ramp, dict(cell=16, range=0.5, blur=1, detail=1.5)), (ramp, dict(cell=64, range=0.5, blur=0)),
                    (ref.planted_image(37, 23)[0], dict(cell=8, blur=4)), (black, dict(cell=8))):
        r.local_tone_image(img, **kw)
        assert r.read_local_tone().tobytes() == pkg.api.local_tone_host(img, **kw).tobytes(), kw
    assert r.read_local_tone().tobytes() == black.tobytes()


# ------------------------------------------------------------------------------------------------------------ the context's images
@pytest.fixture(scope="module")
def box(gpu, pkg, hip_lib):
    """The Cornell box at 64 x 48, 6 subframes of "pt" with the moments and 4 buckets on, then the variance-guided denoiser, the robust
    resolve, a history resolve, bloom of the film and a display call: every source the stage can take and every plane it must keep."""
    assert hip_lib.spcbpt_build_arithmetic().decode() == "ieee"
    w, h = 64, 48
    r = _renderer(pkg, pkg.scenes.cornell_box(), w, h)
    r.set_film_moments(True)
    r.set_film_buckets(4)
    for f in range(FRAMES):
        r.launch("pt", f)
        r.launch_features(f)
    r.denoise_variance()
    r.robust_resolve(1.0)
    r.history_resolve(FRAMES)
    r.bloom("film", strength=0.3)
    r.display("film")
    images = dict(film=r.read_accum().copy(), denoised=r.read_denoised()[0].copy(), robust=r.read_robust()[0].copy(), history=r.read_history()["resolved"].copy(),
                  bloom=r.read_bloom().copy())
    return dict(r=r, w=w, h=h, images=images, before=_planes(r))


def test_sources_match_the_host_form_and_keep_every_other_plane(pkg, box):
    r = box["r"]
    kw = dict(cell=8, range=1.0, blur=1, compress=0.5, detail=1.2)
    for source in SOURCES:
        img = box["images"][source]
        assert np.isfinite(img).all() and img[..., :3].max() > 1e-2
        r.local_tone(source, **kw)
        plane = r.read_local_tone()
        assert plane.shape == (box["h"], box["w"], 4)
        assert plane.tobytes() == pkg.api.local_tone_host(img, **kw).tobytes(), source
        assert plane.tobytes() != img.tobytes()
        r.local_tone(source, **kw)                             # two calls in a row: the same bits
        assert r.read_local_tone().tobytes() == plane.tobytes()
        after = _planes(r)                                     # accum, frame, moments, buckets, the denoised / robust / history outputs, bloom, display
        for k, v in box["before"].items():
            assert after[k] == v, (source, k)


def test_the_plane_feeds_the_display(pkg, box):
    """display("local", ...) is display_host of what read_local_tone returned, outside the quantisation ties."""
    r = box["r"]
    r.local_tone("bloom", compress=0.5)
    plane = r.read_local_tone()
    r.display_reset()
    r.display("local", op="aces", auto=True)
    dev8, ev = r.read_display()
    host8, _, host_ev = pkg.api.display_host(plane, op="aces", auto=True)
    assert dev8.shape == plane.shape and np.float32(ev).tobytes() == np.float32(host_ev).tobytes()
    finite = display_ref.finite_pixels(plane)
    codes = display_ref.tone_codes(plane, ev, "aces")
    display_ref.check_bytes(dev8, codes, finite)
    display_ref.check_bytes(host8, codes, finite)
    assert not (dev8[..., :3][finite] != host8[..., :3][finite])[~tie_mask(codes[finite])].any()
    assert len(np.unique(dev8[..., :3])) > 32
    r.display("film")                                          # the fixture's display plane back, for whoever runs next
    assert r.read_display()[0].tobytes() == box["before"]["display"]


def test_the_span_reports_a_time(pkg, plain):
    r = plain
    img, _ = ref.planted_image(130, 70)
    r.enable_kernel_timing(True)
    r.reset_kernel_time()
    r.local_tone_image(img, blur=4)
    r.sync()
    ms, launches = r.kernel_time("local_tone")
    r.enable_kernel_timing(False)
    assert launches == 1 and ms > 0.0, (ms, launches)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(gpu, pkg):
    r = _renderer(pkg, pkg.scenes.cornell_box(), 48, 32)
    _fails(pkg, r.read_local_tone, STATE, "local_tone")
    _fails(pkg, lambda: r.display("local"), STATE, "spcbpt_local_tone")
    r.launch("pt", 0)
    _fails(pkg, lambda: r.local_tone("robust"), STATE, "buckets")
    _fails(pkg, lambda: r.local_tone("denoised"), STATE, "denoise")
    _fails(pkg, lambda: r.local_tone("history"), STATE, "history_resolve")
    _fails(pkg, lambda: r.local_tone("bloom"), STATE, "spcbpt_bloom")
    r.set_film_buckets(4)
    _fails(pkg, lambda: r.local_tone("robust"), STATE, "robust_resolve")
    r.set_film_buckets(0)
    r.launch_deferred("pt", 1)
    _fails(pkg, lambda: r.local_tone("film"), STATE, "deferred")
    r.merge_deferred(True)
    _fails(pkg, r.read_local_tone, STATE, "local_tone")        # a refused call leaves nothing behind
    nan, inf = float("nan"), float("inf")
    for kw in (dict(cell=3), dict(cell=65), dict(range=0.4), dict(range=8.5), dict(range=nan), dict(blur=-1), dict(blur=5), dict(compress=0.0),
               dict(compress=2.5), dict(compress=inf), dict(detail=-0.5), dict(detail=4.01), dict(detail=nan), dict(anchor=0.0), dict(anchor=-0.18),
               dict(anchor=inf)):
        _fails(pkg, lambda: r.local_tone("film", **kw), INVALID, "local_tone")
        _fails(pkg, lambda: r.local_tone_image(np.ones((2, 2, 4), np.float32), **kw), INVALID, "local_tone")
    _fails(pkg, lambda: r.local_tone(5), INVALID, "source")    # the local plane is no source of its own
    _fails(pkg, lambda: r.local_tone(7), INVALID, "source")
    _fails(pkg, lambda: r.local_tone(-1), INVALID, "source")
    _fails(pkg, lambda: r.display(7), INVALID, "source")
    for s in (4, 5, 7):
        _fails(pkg, lambda: r.bloom(s), INVALID, "source")     # ... and none of spcbpt_bloom
    _fails(pkg, lambda: r.local_tone_image(np.ones((1 << 20, 4, 4), np.float32), cell=4, range=0.5), INVALID, "2^25")   # 2 x 262 145 x 66 nodes
    _fails(pkg, r.read_local_tone, STATE, "local_tone")
    r.local_tone("film")
    assert r.read_local_tone().shape == (32, 48, 4)
    r.display("local")
    assert r.read_display()[0].shape == (32, 48, 4)
    r.resize(48, 32)
    _fails(pkg, r.read_local_tone, STATE, "local_tone")        # a resize drops the plane
    _fails(pkg, lambda: r.display("local"), STATE, "spcbpt_local_tone")
    fresh = pkg.Renderer(pkg.scenes.cornell_box(), 0)
    _fails(pkg, lambda: fresh.local_tone("film"), STATE, "resize")
    fresh.local_tone_image(ref.seeded_image(7, 5))             # an image of the caller's needs no film
    assert fresh.read_local_tone().shape == (5, 7, 4)
    fresh.display("local", op="linear")                        # ... and neither does showing it, at the plane's own size
    assert fresh.read_display()[0].shape == (5, 7, 4)
    fresh.bloom_image(ref.seeded_image(9, 6))
    fresh.local_tone("bloom")                                  # ... nor the glare first: the bloom plane at its own size
    assert fresh.read_local_tone().shape == (6, 9, 4)


# ------------------------------------------------------------------------------------------------------------ the tool
def test_render_tool_shows_the_local_plane(gpu, pkg, tmp_path):
    """tools/spcbpt_render --bloom 0.3 --local-tone 0.5 --local-cell 8 --tone aces --auto-exposure on the Cornell box at 48 x 32:
    <out>_display.ppm holds display_host(local_tone_host(bloom_host(pfm))) outside the ties -- glare first, then the local operator."""
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "spcbpt_render"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    path = pkg.scenes.write_scene(pkg.scenes.cornell_box(), str(tmp_path), "cornell")
    w, h = 48, 32
    out = os.path.join(str(tmp_path), "shown")
    cmd = [os.path.join(ROOT, "tools", "spcbpt_render"), path, str(tmp_path), "--alg", "pt", f"--dim={w}x{h}", "--frames", "4", "--out", out,
           "--bloom", "0.3", "--local-tone", "0.5", "--local-cell", "8", "--tone", "aces", "--auto-exposure"]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0 and "through spcbpt_local_tone: compress 0.5, detail 1, cell 8, range 1" in p.stdout, p.stdout[-3000:]
    raw = open(out + ".pfm", "rb").read().split(b"\n", 3)
    assert raw[0] == b"PF" and raw[1] == b"%d %d" % (w, h)
    img = np.ones((h, w, 4), np.float32)
    img[..., :3] = np.frombuffer(raw[3], np.float32).reshape(h, w, 3)          # bottom row first, like accum
    head = b"P6\n%d %d\n255\n" % (w, h)
    ppm = open(out + "_display.ppm", "rb").read()
    assert ppm.startswith(head) and len(ppm) == len(head) + w * h * 3
    tool8 = np.full((h, w, 4), 255, np.uint8)
    tool8[..., :3] = np.frombuffer(ppm[len(head):], np.uint8).reshape(h, w, 3)[::-1]   # the PPM is top row first
    plane = pkg.api.local_tone_host(pkg.api.bloom_host(img, strength=0.3), compress=0.5, cell=8)
    host8, _, host_ev = pkg.api.display_host(plane, op="aces", auto=True)
    codes = display_ref.tone_codes(plane, host_ev, "aces")
    finite = display_ref.finite_pixels(plane)
    display_ref.check_bytes(tool8, codes, finite)
    display_ref.check_bytes(host8, codes, finite)
    assert not (tool8[..., :3][finite] != host8[..., :3][finite])[~tie_mask(codes[finite])].any()
    assert len(np.unique(tool8[..., :3])) > 32
