"""The display transform on the device (spcbpt_display, spcbpt_display_image): its RGBA8 plane, histogram and EV against the host form
spcbpt_display_host run on the float image read back -- histogram equal as integers, EV equal as float32 bits (only + - x / are on its
path; the library under test is the IEEE build), RGBA8 equal outside the quantisation ties of tests/display_ref.py (the device's
powf / exp2f and the host's differ in the last bits) and both held to the float64 codes --, that operator 0 at EV 0 is read_frame()
byte for byte, that every other plane keeps its bits, the adaptation state, and what is refused.

Measured on the MI355X: see DESIGN.md 8j."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import display_ref as ref
from tests.test_gpu_mesh_light import _renderer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE, INVALID = -5, -1
FRAMES = 6


def _fails(pkg, fn, code, text=None):
    with pytest.raises(pkg.SpcbptError) as e:
        fn()
    assert f"({code})" in str(e.value), str(e.value)
    if text:
        assert text in str(e.value), str(e.value)


def _bits(x):
    return struct.pack("<f", x)


def _planes(r):
    """Every plane a display call must leave alone, as bytes."""
    den, den8 = r.read_denoised()
    rob, rob8 = r.read_robust()
    hist = r.read_history()
    return dict(accum=r.read_accum().tobytes(), frame=r.read_frame().tobytes(), moments=r.read_film_moments().tobytes(), buckets=r.read_film_buckets().tobytes(),
                denoised=den.tobytes(), denoised8=den8.tobytes(), robust=rob.tobytes(), robust8=rob8.tobytes(),
                resolved=hist["resolved"].tobytes(), resolved8=hist["frame"].tobytes())


@pytest.fixture(scope="module", params=[(48, 32), (43, 29)], ids=["48x32", "43x29"])
def box(request, gpu, pkg, hip_lib):
    """The Cornell box, 6 subframes of "pt" with the moments and 4 buckets on, then the variance-guided denoiser, the robust resolve and a
    history resolve: every source the pass can show."""
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


def _against_host(pkg, r, img, what, **params):
    """The last display call's plane, histogram (if it has one) and EV against spcbpt_display_host on `img`, and both against the float64
    codes.  Returns (rgba8, hist, ev)."""
    dev8, ev = r.read_display()
    assert dev8.shape == img.shape
    want_hist = params.get("auto") or params.get("histogram")
    host8, host_hist, host_ev = pkg.api.display_host(img, **params)
    hist = None
    if want_hist:
        hist = r.read_display_histogram()
        assert int(hist.astype(np.int64).sum()) == img.shape[0] * img.shape[1]
        assert hist.tolist() == host_hist.tolist(), what
    assert _bits(ev) == _bits(host_ev), (what, ev, host_ev)
    finite = ref.finite_pixels(img)
    codes = ref.tone_codes(img, ev, params.get("op", "film"), params.get("white", 4.0))
    ties, dev_differ = ref.check_bytes(dev8, codes, finite)
    _, host_differ = ref.check_bytes(host8, codes, finite)
    tie = ref.tie_mask(codes[finite])
    unequal = dev8[..., :3][finite] != host8[..., :3][finite]
    print(f"{what}: EV {ev:.6f}; {ties} of {codes[finite].size} values at a tie (cap {ref.tie_cap(codes[finite].size)}); off the float64 byte: device {dev_differ}, "
          f"host {host_differ}; device != host at {int(unequal.sum())} values, all ties: {not unequal[~tie].any()}")
    assert not unequal[~tie].any()
    return dev8, hist, ev


# ------------------------------------------------------------------------------------------------------------ the context's images
def test_default_operator_is_the_frame(box):
    r = box["r"]
    r.display("film", op="film", ev=0.0)
    out8, ev = r.read_display()
    assert ev == 0.0 and out8.shape == (box["h"], box["w"], 4)
    assert out8.tobytes() == box["before"]["frame"]
    r.display("film")                                  # the defaults are that call
    assert r.read_display()[0].tobytes() == box["before"]["frame"]


@pytest.mark.parametrize("source", ["film", "denoised", "robust", "history"])
def test_sources_match_the_host_form(pkg, box, source):
    r, img = box["r"], box["images"][source]
    assert np.isfinite(img).all() and img[..., :3].max() > 1e-2
    r.display_reset()
    for op in ref.OPS:
        r.display(source, op=op, auto=True)
        out8, hist, ev = _against_host(pkg, r, img, f"{box['w']}x{box['h']} {source}, {op}, auto", op=op, auto=True)
        assert len(np.unique(out8[..., :3])) > 32
        # two identical calls return the same bytes, the same histogram and the same EV
        r.display(source, op=op, auto=True)
        again8, again_ev = r.read_display()
        assert again8.tobytes() == out8.tobytes() and _bits(again_ev) == _bits(ev) and r.read_display_histogram().tolist() == hist.tolist()
    r.display(source, op="reinhard", ev=1.5, white=2.0, histogram=True)
    _against_host(pkg, r, img, f"{box['w']}x{box['h']} {source}, reinhard, EV 1.5", op="reinhard", ev=1.5, white=2.0, histogram=True)
    r.display(source, op="aces", ev=-1.0)
    _against_host(pkg, r, img, f"{box['w']}x{box['h']} {source}, aces, EV -1", op="aces", ev=-1.0)
    # accum, frame, the moments, the buckets, the denoised, robust and resolved outputs are bit for bit what they were
    after = _planes(r)
    for k, v in box["before"].items():
        assert after[k] == v, k


def test_histogram_does_not_depend_on_the_way_in(pkg, box):
    r = box["r"]
    r.display("film", auto=True)
    h0, (b0, e0) = r.read_display_histogram(), r.read_display()
    r.display_image(r.read_accum(), auto=True)
    h1, (b1, e1) = r.read_display_histogram(), r.read_display()
    assert h0.tolist() == h1.tolist() and _bits(e0) == _bits(e1) and b0.tobytes() == b1.tobytes()
    assert r.read_accum().tobytes() == box["before"]["accum"] and r.read_frame().tobytes() == box["before"]["frame"]


# ------------------------------------------------------------------------------------------------------------ images of the caller's
@pytest.fixture(scope="module")
def plain(gpu, pkg):
    return _renderer(pkg, pkg.scenes.cornell_box(), 48, 32)


@pytest.mark.parametrize("name", ["257x3", "7x5", "1x1", "edges", "1201x901"])
def test_display_image_matches_the_host_form(pkg, plain, name):
    """The shapes where a grid-stride bound, the flush of a partly filled block or the outer counters go wrong.  1201 x 901 is more
    pixels than one trip of the histogram's loop holds (1 024 blocks x 256 lanes x 4 loads = 1 048 576): the first lanes make a second
    trip whose four loads are ragged; it runs one operator, the others change nothing in that loop."""
    r = plain
    big = name == "1201x901"
    if name == "edges":
        img = ref.edges_image()[0]
    else:
        w, h = (int(v) for v in name.split("x"))
        img = ref.seeded_image(w, h)
    r.display_reset()
    for op in (("aces",) if big else ref.OPS):
        r.display_image(img, op=op, auto=True)
        _, hist, ev = _against_host(pkg, r, img, f"image {name}, {op}, auto", op=op, auto=True)
    assert hist.tolist() == ref.histogram(img).tolist()
    if big:
        return
    if name == "edges":
        assert int(hist[ref.DARK]) == 5 and int(hist[ref.BRIGHT]) == 2
    r.display_image(img, op="linear", ev=3.0, histogram=True)
    _against_host(pkg, r, img, f"image {name}, linear, EV 3", op="linear", ev=3.0, histogram=True)
    r.display_image(img, op="film", ev=-2.0)
    _against_host(pkg, r, img, f"image {name}, film, EV -2", op="film", ev=-2.0)
    assert r.image_size() == (48, 32)                      # the context's film keeps its size


# ------------------------------------------------------------------------------------------------------------ adaptation
def test_adaptation_state_lives_on_the_device(pkg, plain):
    r = plain
    a = ref.seeded_image(43, 29)
    b = a.copy()
    b[..., :3] *= np.float32(8.0)
    kw = dict(auto=True, adapt=0.5, op="reinhard")

    def run(images, have, prev):
        dev, host = [], []
        for img in images:
            r.display_image(img, **kw)
            dev.append(r.read_display()[1])
            prev = pkg.api.display_host(img, have_prev=have, prev_ev=prev, **kw)[2]   # the host form, fed its own previous EV
            have = True
            host.append(prev)
        assert [_bits(v) for v in dev] == [_bits(v) for v in host], (dev, host)
        return dev

    r.display_reset()
    first = run([a, a, a], False, 0.0)
    assert first[0] == first[1] == first[2]                # one image: the first call jumps to the target and stays
    moved = run([b, b, b], True, first[-1])                # three stops brighter: half of what is left per call
    steps = np.diff([first[-1]] + moved)
    assert np.allclose(steps, [-1.5, -0.75, -0.375], atol=1e-5), steps
    r.display_image(a, ev=2.0, op="aces")                  # a manual call neither reads nor writes the state
    assert r.read_display()[1] == 2.0
    assert run([b], True, moved[-1])[0] != moved[-1]
    r.display_reset()
    assert run([a], False, 0.0)[0] == first[0]             # display_reset brings back the first value
    run([b], True, first[0])
    r.resize(48, 32)
    _fails(pkg, r.read_display, STATE, "display")          # a resize drops the plane ...
    assert run([a], False, 0.0)[0] == first[0]             # ... and the previous EV


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(gpu, pkg):
    r = _renderer(pkg, pkg.scenes.cornell_box(), 48, 32)
    _fails(pkg, r.read_display, STATE, "display")
    _fails(pkg, r.read_display_histogram, STATE, "display")
    r.launch("pt", 0)
    _fails(pkg, lambda: r.display("robust"), STATE, "buckets")
    _fails(pkg, lambda: r.display("denoised"), STATE, "denoise")
    _fails(pkg, lambda: r.display("history"), STATE, "history_resolve")
    r.set_film_buckets(4)
    _fails(pkg, lambda: r.display("robust"), STATE, "robust_resolve")
    r.set_film_buckets(0)
    r.launch_deferred("pt", 1)
    _fails(pkg, lambda: r.display("film"), STATE, "deferred")
    r.merge_deferred(True)
    _fails(pkg, r.read_display, STATE, "display")          # a refused call leaves nothing behind
    r.display("film", ev=1.0)
    assert r.read_display()[1] == 1.0
    _fails(pkg, r.read_display_histogram, STATE, "histogram")
    r.display("film", ev=1.0, histogram=True)
    assert int(r.read_display_histogram().astype(np.int64).sum()) == 48 * 32
    for kw in (dict(op=4), dict(op=-1), dict(low_fraction=0.6, high_fraction=0.5), dict(low_fraction=1.0), dict(ev_min=1.0, ev_max=0.0), dict(adapt=0.0),
               dict(adapt=1.25), dict(key=float("nan")), dict(ev=float("inf")), dict(white=0.0), dict(flags=8)):
        _fails(pkg, lambda: r.display("film", **kw), INVALID, "display")
        _fails(pkg, lambda: r.display_image(np.ones((2, 2, 4), np.float32), **kw), INVALID, "display")
    _fails(pkg, lambda: r.display(7), INVALID, "source")
    fresh = pkg.Renderer(pkg.scenes.cornell_box(), 0)
    _fails(pkg, lambda: fresh.display("film"), STATE, "resize")
    fresh.display_image(ref.seeded_image(7, 5), auto=True)     # an image of the caller's needs no film
    assert fresh.read_display()[0].shape == (5, 7, 4)


# ------------------------------------------------------------------------------------------------------------ the tool
def test_render_tool_writes_the_display_image(gpu, pkg, tmp_path):
    """tools/spcbpt_render --auto-exposure --tone aces on the Cornell box at 48 x 32: <out>_display.ppm holds spcbpt_display_host's bytes
    of the PFM the run wrote (outside the ties), at the EV it printed; <out>.ppm is what the run writes without the flags."""
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "spcbpt_render"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    path = pkg.scenes.write_scene(pkg.scenes.cornell_box(), str(tmp_path), "cornell")
    w, h = 48, 32
    outs = {}
    for tag, extra in (("plain", []), ("shown", ["--auto-exposure", "--tone", "aces"])):
        out = os.path.join(str(tmp_path), tag)
        cmd = [os.path.join(ROOT, "tools", "spcbpt_render"), path, str(tmp_path), "--alg", "pt", f"--dim={w}x{h}", "--frames", "4", "--out", out] + extra
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-3000:]
        outs[tag] = (out, p.stdout)
    plain, shown = outs["plain"][0], outs["shown"][0]
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
    host8, _, host_ev = pkg.api.display_host(img, op="aces", auto=True)
    m = re.search(r"_display\.ppm.*EV ([-+0-9.eE]+)", outs["shown"][1])
    assert m, outs["shown"][1][-2000:]
    assert _bits(float(m.group(1))) == _bits(host_ev)
    codes = ref.tone_codes(img, host_ev, "aces")
    finite = ref.finite_pixels(img)
    ref.check_bytes(tool8, codes, finite)
    ref.check_bytes(host8, codes, finite)
    tie = ref.tie_mask(codes[finite])
    assert not (tool8[..., :3][finite] != host8[..., :3][finite])[~tie].any()
    assert len(np.unique(tool8[..., :3])) > 32
