"""The bloom stage on the device (spcbpt_bloom, spcbpt_bloom_image): its float4 plane against the host form spcbpt_bloom_host run on the
same image -- BIT FOR BIT: only + - x /, min and compare are on the path and the library under test is the IEEE build, whichever
way the pyramid is cut between the per-level kernels and the fused tail --, the plane as a display source, that every other plane keeps
its bits, and what is refused.  The host form is held to the float64 definition by tests/test_bloom_host.py.

Measured on the MI355X: see DESIGN.md 8k."""
import os
import subprocess

import numpy as np
import pytest

from tests import bloom_ref as ref
from tests import display_ref
from tests.display_ref import tie_mask
from tests.test_gpu_mesh_light import _renderer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, INVALID = -5, -1
FRAMES = 6
GRID = [(L, q, T) for L in ref.LEVELS for q in ref.SPREADS for T in ref.THRESHOLDS]
SOURCES = ("film", "denoised", "robust", "history")


def _fails(pkg, fn, code, text=None):
    with pytest.raises(pkg.SpcbptError) as e:
        fn()
    assert f"({code})" in str(e.value), str(e.value)
    if text:
        assert text in str(e.value), str(e.value)


def _planes(r):
    """Every plane a bloom call must leave alone, as bytes (the list of tests/test_gpu_display.py)."""
    den, den8 = r.read_denoised()
    rob, rob8 = r.read_robust()
    hist = r.read_history()
    return dict(accum=r.read_accum().tobytes(), frame=r.read_frame().tobytes(), moments=r.read_film_moments().tobytes(), buckets=r.read_film_buckets().tobytes(),
                denoised=den.tobytes(), denoised8=den8.tobytes(), robust=rob.tobytes(), robust8=rob8.tobytes(),
                resolved=hist["resolved"].tobytes(), resolved8=hist["frame"].tobytes())


@pytest.fixture(scope="module")
def plain(gpu, pkg, hip_lib):
    assert hip_lib.spcbpt_build_arithmetic().decode() == "ieee"
    return _renderer(pkg, pkg.scenes.cornell_box(), 48, 32)


# ------------------------------------------------------------------------------------------------------------ images of the caller's
@pytest.mark.parametrize("name", [f"{w}x{h}" for w, h in ref.SIZES])
def test_bloom_image_is_the_host_form_bit_for_bit(pkg, plain, name):
    """130 x 67: a second workgroup and a ragged last wave in x; 7 x 5 and 9 x 1: levels that collapse to one texel while others remain;
    1 x 1: clamped addressing with nothing to clamp to.  All of these run the level-0 down pass, the fused tail and the composite."""
    r = plain
    w, h = (int(v) for v in name.split("x"))
    img, plants = ref.planted_image(w, h)
    for L, q, T in GRID:
        kw = dict(levels=L, strength=0.7, spread=q, threshold=T)
        r.bloom_image(img, **kw)
        dev = r.read_bloom()
        assert dev.shape == img.shape and dev.dtype == np.float32
        assert dev.tobytes() == pkg.api.bloom_host(img, **kw).tobytes(), (name, kw)
    r.bloom_image(img, **kw)                                   # the same call twice: the same bytes
    assert r.read_bloom().tobytes() == dev.tobytes()
    for (y, x, c) in plants["nan"]:
        assert np.isnan(dev[y, x, c])
    assert int(np.isnan(dev).sum()) == len(plants["nan"])
    assert r.image_size() == (48, 32)                          # the context's film keeps its size


@pytest.mark.parametrize("name,L", [("300x200", 3), ("400x300", 2), ("300x200", 1)])
def test_every_launch_structure_returns_the_same_bits(pkg, plain, monkeypatch, name, L):
    """The sizes at which the stage takes another path.  300 x 200, L = 3: the levels 150 x 100 and 75 x 50 are made by the tiled down
    kernel (the second by its form without the threshold step), the tail takes over at level 2 and an up pass brings level 1 back.
    400 x 300, L = 2: the coarsest level (100 x 75) does not fit the tail: per-level kernels only.  L = 1: one down pass and the composite.
    With the tail switched off (SPCBPT_BLOOM_TAIL=0, the switch the two forms were measured with) the bytes are the same."""
    r = plain
    w, h = (int(v) for v in name.split("x"))
    img, _ = ref.planted_image(w, h)
    kw = dict(levels=L, strength=0.4, spread=2.0, threshold=0.5)
    want = pkg.api.bloom_host(img, **kw).tobytes()
    r.bloom_image(img, **kw)
    assert r.read_bloom().tobytes() == want
    monkeypatch.setenv("SPCBPT_BLOOM_TAIL", "0")
    r.bloom_image(img, **kw)
    assert r.read_bloom().tobytes() == want
    small, _ = ref.planted_image(43, 29)
    r.bloom_image(small, levels=8, strength=0.7)
    assert r.read_bloom().tobytes() == pkg.api.bloom_host(small, levels=8, strength=0.7).tobytes()


# ------------------------------------------------------------------------------------------------------------ the context's images
@pytest.fixture(scope="module", params=[(48, 32), (43, 29)], ids=["48x32", "43x29"])
def box(request, gpu, pkg, hip_lib):
    """The Cornell box, 6 subframes of "pt" with the moments and 4 buckets on, then the variance-guided denoiser, the robust resolve and a
    history resolve: every source the stage can take (the fixture of tests/test_gpu_display.py)."""
    assert hip_lib.spcbpt_build_arithmetic().decode() == "ieee"
    w, h = request.param
    r = _renderer(pkg, pkg.scenes.cornell_box(), w, h)
    r.set_film_moments(True)
    r.set_film_buckets(4)
    for f in range(FRAMES):
        r.launch("pt", f)
        r.launch_features(f)
    r.denoise_variance()
    r.robust_resolve(1.0)
    r.history_resolve(FRAMES)
    images = dict(film=r.read_accum().copy(), denoised=r.read_denoised()[0].copy(), robust=r.read_robust()[0].copy(), history=r.read_history()["resolved"].copy())
    return dict(r=r, w=w, h=h, images=images, before=_planes(r))


def test_sources_match_the_host_form_and_feed_the_display(pkg, box):
    r = box["r"]
    for source in SOURCES:
        img = box["images"][source]
        assert np.isfinite(img).all() and img[..., :3].max() > 1e-2
        kw = dict(levels=4, strength=0.3, threshold=0.25)
        r.bloom(source, **kw)
        plane = r.read_bloom()
        assert plane.shape == (box["h"], box["w"], 4)
        assert plane.tobytes() == pkg.api.bloom_host(img, **kw).tobytes(), source
        assert plane.tobytes() != img.tobytes()
        # the plane as a display source: display_host of what read_bloom returned, outside the quantisation ties
        r.display_reset()
        r.display("bloom", op="aces", auto=True)
        dev8, ev = r.read_display()
        host8, _, host_ev = pkg.api.display_host(plane, op="aces", auto=True)
        assert dev8.shape == plane.shape and np.float32(ev).tobytes() == np.float32(host_ev).tobytes()
        finite = display_ref.finite_pixels(plane)
        codes = display_ref.tone_codes(plane, ev, "aces")
        display_ref.check_bytes(dev8, codes, finite)
        display_ref.check_bytes(host8, codes, finite)
        assert not (dev8[..., :3][finite] != host8[..., :3][finite])[~tie_mask(codes[finite])].any()
        assert len(np.unique(dev8[..., :3])) > 32
    # accum, frame, the moments, the buckets, the denoised, robust and resolved outputs are bit for bit what they were
    after = _planes(r)
    for k, v in box["before"].items():
        assert after[k] == v, k
    r.display("film")
    assert r.read_display()[0].tobytes() == r.read_frame().tobytes() == box["before"]["frame"]


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(gpu, pkg):
    r = _renderer(pkg, pkg.scenes.cornell_box(), 48, 32)
    _fails(pkg, r.read_bloom, STATE, "bloom")
    _fails(pkg, lambda: r.display("bloom"), STATE, "spcbpt_bloom")
    r.launch("pt", 0)
    _fails(pkg, lambda: r.bloom("robust"), STATE, "buckets")
    _fails(pkg, lambda: r.bloom("denoised"), STATE, "denoise")
    _fails(pkg, lambda: r.bloom("history"), STATE, "history_resolve")
    r.set_film_buckets(4)
    _fails(pkg, lambda: r.bloom("robust"), STATE, "robust_resolve")
    r.set_film_buckets(0)
    r.launch_deferred("pt", 1)
    _fails(pkg, lambda: r.bloom("film"), STATE, "deferred")
    r.merge_deferred(True)
    _fails(pkg, r.read_bloom, STATE, "bloom")                  # a refused call leaves nothing behind
    nan, inf = float("nan"), float("inf")
    for kw in (dict(levels=0), dict(levels=9), dict(strength=-0.5), dict(strength=1.01), dict(strength=nan), dict(spread=0.0), dict(spread=4.01),
               dict(spread=inf), dict(threshold=-1e-3), dict(threshold=inf), dict(clamp=0.0), dict(clamp=3.0e19), dict(clamp=nan)):
        _fails(pkg, lambda: r.bloom("film", **kw), INVALID, "bloom")
        _fails(pkg, lambda: r.bloom_image(np.ones((2, 2, 4), np.float32), **kw), INVALID, "bloom")
    _fails(pkg, lambda: r.bloom(4), INVALID, "source")           # the bloom plane is no source of its own
    _fails(pkg, lambda: r.bloom(7), INVALID, "source")
    _fails(pkg, lambda: r.display(7), INVALID, "source")
    _fails(pkg, r.read_bloom, STATE, "bloom")
    r.bloom("film")
    assert r.read_bloom().shape == (32, 48, 4)
    r.display("bloom")
    assert r.read_display()[0].shape == (32, 48, 4)
    r.resize(48, 32)
    _fails(pkg, r.read_bloom, STATE, "bloom")                  # a resize drops the plane
    _fails(pkg, lambda: r.display("bloom"), STATE, "spcbpt_bloom")
    fresh = pkg.Renderer(pkg.scenes.cornell_box(), 0)
    _fails(pkg, lambda: fresh.bloom("film"), STATE, "resize")
    fresh.bloom_image(ref.seeded_image(7, 5))                  # an image of the caller's needs no film
    assert fresh.read_bloom().shape == (5, 7, 4)
    fresh.display("bloom", op="linear")                        # ... and neither does showing it, at the plane's own size
    assert fresh.read_display()[0].shape == (5, 7, 4)


# ------------------------------------------------------------------------------------------------------------ the tool
def test_render_tool_shows_the_bloom_plane(gpu, pkg, tmp_path):
    """tools/spcbpt_render --bloom 0.3 --tone aces --auto-exposure on the Cornell box at 48 x 32: <out>_display.ppm holds
    display_host(bloom_host(pfm)) outside the ties; <out>.pfm and <out>.ppm are what the run writes without the flags."""
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "spcbpt_render"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    path = pkg.scenes.write_scene(pkg.scenes.cornell_box(), str(tmp_path), "cornell")
    w, h = 48, 32
    outs = {}
    for tag, extra in (("plain", []), ("shown", ["--bloom", "0.3", "--tone", "aces", "--auto-exposure"])):
        out = os.path.join(str(tmp_path), tag)
        cmd = [os.path.join(ROOT, "tools", "spcbpt_render"), path, str(tmp_path), "--alg", "pt", f"--dim={w}x{h}", "--frames", "4", "--out", out] + extra
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-3000:]
        outs[tag] = out
    plain, shown = outs["plain"], outs["shown"]
    assert not os.path.exists(plain + "_display.ppm")
    assert open(plain + ".ppm", "rb").read() == open(shown + ".ppm", "rb").read()
    assert open(plain + ".pfm", "rb").read() == open(shown + ".pfm", "rb").read()
    raw = open(shown + ".pfm", "rb").read().split(b"\n", 3)
    assert raw[0] == b"PF" and raw[1] == b"%d %d" % (w, h)
    img = np.ones((h, w, 4), np.float32)
    img[..., :3] = np.frombuffer(raw[3], np.float32).reshape(h, w, 3)          # bottom row first, like accum
    head = b"P6\n%d %d\n255\n" % (w, h)
    ppm = open(shown + "_display.ppm", "rb").read()
    assert ppm.startswith(head) and len(ppm) == len(head) + w * h * 3
    tool8 = np.full((h, w, 4), 255, np.uint8)
    tool8[..., :3] = np.frombuffer(ppm[len(head):], np.uint8).reshape(h, w, 3)[::-1]   # the PPM is top row first
    plane = pkg.api.bloom_host(img, strength=0.3)
    host8, _, host_ev = pkg.api.display_host(plane, op="aces", auto=True)
    codes = display_ref.tone_codes(plane, host_ev, "aces")
    finite = display_ref.finite_pixels(plane)
    display_ref.check_bytes(tool8, codes, finite)
    display_ref.check_bytes(host8, codes, finite)
    assert not (tool8[..., :3][finite] != host8[..., :3][finite])[~tie_mask(codes[finite])].any()
    assert len(np.unique(tool8[..., :3])) > 32
