"""The bucket film on the device (spcbpt_set_film_buckets) and its median-of-means resolve (spcbpt_robust_resolve): the planes against an
exact float32 replay of the film and against the host form byte for byte, the resolve against the host form (w equal at every pixel,
rgb within 1e-5 of the pixel's largest channel -- DESIGN.md 8e's bar; the library under test is the IEEE build), that a context which
does not ask keeps its film bits, which launches count, and what is refused.

Measured on the MI355X: see DESIGN.md 8i."""
import numpy as np
import pytest

from tests.denoise_ref import tone_map_codes
from tests.test_gpu_mesh_light import _renderer

pytestmark = pytest.mark.gpu

STATE, INVALID = -5, -1
FRAMES = 11          # in 4 buckets: 3, 3, 3, 2


def _fails(pkg, fn, code, text=None):
    with pytest.raises(pkg.SpcbptError) as e:
        fn()
    assert f"({code})" in str(e.value), str(e.value)
    if text:
        assert text in str(e.value), str(e.value)


@pytest.fixture(scope="module", params=[(48, 32), (43, 29)], ids=["48x32", "43x29"])
def box(request, gpu, pkg, hip_lib):
    """The Cornell box, 11 subframes of "pt" on three contexts: A with K = 32 (every bucket holds one sample), B with K = 4 and the
    moments on, and one with the switch off."""
    assert hip_lib.spcbpt_build_arithmetic().decode() == "ieee"
    w, h = request.param
    scene = pkg.scenes.cornell_box()
    a, b, off = (_renderer(pkg, scene, w, h) for _ in range(3))
    assert a.film_buckets() == 0
    a.set_film_buckets(32)
    b.set_film_buckets(4)
    b.set_film_moments(True)
    assert a.film_buckets() == 32 and b.film_buckets() == 4 and off.film_buckets() == 0
    films, first = [], None
    for f in range(FRAMES):
        for r in (a, b, off):
            r.launch("pt", f)
        films.append(a.read_accum().copy())
        if f == 0:
            first = a.read_film_buckets().copy()
    return dict(a=a, b=b, off=off, w=w, h=h, films=films, first=first, planes_a=a.read_film_buckets().copy(), planes_b=b.read_film_buckets().copy(),
                accum=b.read_accum().copy(), frame=b.read_frame().copy(), m2n=b.read_film_moments().copy())


def test_buckets_replay_the_film_exactly(box):
    """K = 32 and 11 frames: bucket f is frame f's sample, so the film's own running mean over them, in float32, is accum bit for bit."""
    pl, films = box["planes_a"], box["films"]
    assert pl.shape == (32, box["h"], box["w"], 4)
    assert np.all(pl[:FRAMES, ..., 3] == 1) and not pl[FRAMES:].any()
    first = box["first"]
    assert first[0, ..., :3].tobytes() == films[0][..., :3].tobytes() and np.all(first[0, ..., 3] == 1) and not first[1:].any()
    acc = pl[0, ..., :3].copy()
    assert acc.tobytes() == films[0][..., :3].tobytes()
    for f in range(1, FRAMES):
        a = np.float32(1.0) / np.float32(f + 1)
        acc = acc + a * (pl[f, ..., :3] - acc)           # film_write's lerp3, float32 operation for operation
        assert acc.dtype == np.float32 and acc.tobytes() == films[f][..., :3].tobytes(), f
    assert pl[:FRAMES, ..., :3].max() > 1e-2


def test_planes_equal_the_host_form(pkg, box):
    """K = 4: the device's planes are spcbpt_film_buckets_update_host's over the twin's samples, byte for byte."""
    samples = box["planes_a"][:FRAMES]
    host = np.zeros((4, box["h"], box["w"], 4), np.float32)
    for f in range(FRAMES):
        pkg.api.film_buckets_update_host(samples[f], f, host)
    dev = box["planes_b"]
    assert [int(v) for v in dev[:, 0, 0, 3]] == [3, 3, 3, 2]
    assert all(np.all(dev[k, ..., 3] == n) for k, n in enumerate((3, 3, 3, 2)))
    assert dev.tobytes() == host.tobytes()


def test_film_bits_do_not_depend_on_the_switch(pkg, box):
    off = box["off"]
    assert off.read_accum().tobytes() == box["accum"].tobytes() and off.read_frame().tobytes() == box["frame"].tobytes()
    assert box["a"].read_accum().tobytes() == box["accum"].tobytes()
    for fn in (off.read_film_buckets, off.robust_resolve, off.read_robust):
        _fails(pkg, fn, STATE, "buckets")


@pytest.mark.parametrize("strength", [0.0, 1.0, 4.0])
def test_resolve_matches_the_host_form(pkg, box, strength):
    b = box["b"]
    b.robust_resolve(strength)
    out, out8 = b.read_robust()
    host = pkg.api.robust_resolve_host(box["planes_b"], strength)
    assert np.isfinite(out).all()
    differ = int((out[..., 3] != host[..., 3]).sum())
    top = host[..., :3].max(axis=-1)
    dev = np.abs(out[..., :3].astype(np.float64) - host[..., :3]).max(axis=-1)
    rel = float((dev[top > 0] / top[top > 0]).max())
    print(f"{box['w']}x{box['h']}, strength {strength}: w differs at {differ} pixels, kept {sorted(set(int(v) for v in host[..., 3].ravel()))}; "
          f"largest |device - host| {rel:.3e} of the pixel's largest channel (bar 1e-5), bits equal: {out.tobytes() == host.tobytes()}")
    assert differ == 0
    assert np.all(dev <= 1e-5 * top)
    if strength == 0.0:   # 0 is the film: all four buckets, weighted by their counts
        acc = box["accum"][..., :3].astype(np.float64)
        atop = acc.max(axis=-1)
        d0 = np.abs(out[..., :3] - acc).max(axis=-1)
        print(f"    strength 0 against accum: {float((d0[atop > 0] / atop[atop > 0]).max()):.3e} of the pixel's largest channel (bar 1e-5)")
        assert np.all(out[..., 3] == 4) and np.all(d0 <= 1e-5 * atop)
    # two calls return the same bytes
    b.robust_resolve(strength)
    again, again8 = b.read_robust()
    assert again.tobytes() == out.tobytes() and again8.tobytes() == out8.tobytes()
    # accum, frame, the buckets and the moments are bit for bit what they were
    assert b.read_accum().tobytes() == box["accum"].tobytes() and b.read_frame().tobytes() == box["frame"].tobytes()
    assert b.read_film_buckets().tobytes() == box["planes_b"].tobytes() and b.read_film_moments().tobytes() == box["m2n"].tobytes()
    # the RGBA8 output is the film's tone map of the float output: +-1 code where the float64 value sits at a quantisation tie
    codes = tone_map_codes(out[..., :3])
    want = np.minimum(np.floor(codes), 255)
    diff = out8[..., :3].astype(np.int64) - want
    tie = np.abs(codes - np.round(codes)) < 1e-3
    assert (out8[..., 3] == 255).all()
    assert (diff[~tie] == 0).all() and (np.abs(diff) <= 1).all(), (np.abs(diff).max(), int((diff != 0).sum()))


# ------------------------------------------------------------------------------------------------------------ which launches count
def test_bands_restart_deferred_clear_and_resize(gpu, pkg):
    scene = pkg.scenes.cornell_box()
    w, h, K = 43, 29, 5
    r = _renderer(pkg, scene, w, h, tuple_="minimal")
    r.set_film_buckets(K)
    assert r.read_film_buckets().shape == (K, h, w, 4) and not r.read_film_buckets().any()   # before the first merge: zeros
    r.robust_resolve()                                                                         # ... and so is the resolved image
    assert not r.read_robust()[0].any()
    n = lambda: r.read_film_buckets()[..., 3]
    total = lambda: n().sum(axis=0)
    r.launch("pt", 0)
    r.launch("pt", 1)
    assert np.all(n()[:2] == 1) and not n()[2:].any()
    # a banded launch raises n on its rows only: bands 1 and 3 of rows (8, h, 2)
    r.launch("pt", 2, (8, h, 2))
    rows = np.zeros(h, bool)
    rows[8:16] = True
    rows[24:h] = True
    assert np.all(n()[2][rows] == 1) and not n()[2][~rows].any() and np.all(n()[:2] == 1)
    # a deferred frame counts when it is kept and not when it is dropped
    before = r.read_film_buckets().copy()
    r.launch_deferred("pt", 3)
    r.merge_deferred(False)
    assert r.read_film_buckets().tobytes() == before.tobytes()
    r.launch_deferred("pt", 3)
    r.merge_deferred(True)
    assert np.all(n()[3] == 1) and np.all(total() == before[..., 3].sum(axis=0) + 1)
    # "SPCBPT_eye" and "lt" end in the same merge: subframes 4 and 5 -> buckets 4 and 0
    r.render_frame("SPCBPT_eye", 4)
    r.render_frame("lt", 5)
    assert np.all(n()[4] == 1) and np.all(n()[0] == 2) and np.all(total() == before[..., 3].sum(axis=0) + 3)
    # subframe 0 restarts all K buckets
    r.launch("pt", 0)
    m = r.read_film_buckets()
    assert np.all(m[0, ..., 3] == 1) and not m[1:].any()
    assert m[0, ..., :3].tobytes() == r.read_accum()[..., :3].tobytes()
    r.launch("pt", 1)
    r.clear_accum()
    assert not r.read_film_buckets().any()
    r.launch("pt", 0)
    r.robust_resolve()
    r.resize(w, h)
    assert not r.read_film_buckets().any() and r.film_buckets() == K     # a resize forgets the planes, not K
    _fails(pkg, r.read_robust, STATE, "robust_resolve")                  # ... and the resolved image
    r.launch("pt", 0)
    r.launch("pt", 1)
    assert np.all(total() == 2)
    r.set_film_buckets(7)                                                # changing K restarts
    assert r.read_film_buckets().shape == (7, h, w, 4) and not r.read_film_buckets().any()
    r.launch("pt", 9)                                                    # switched on in mid-film: the buckets count the merges since
    assert np.all(n()[9 % 7] == 1) and np.all(total() == 1)
    r.set_film_buckets(0)
    _fails(pkg, r.read_film_buckets, STATE, "buckets")


def test_refusals(gpu, pkg):
    scene = pkg.scenes.cornell_box()
    r = _renderer(pkg, scene, 48, 32, tuple_="minimal")
    for k in (1, 2, 33, -1):
        _fails(pkg, lambda: r.set_film_buckets(k), INVALID, "buckets")
    assert r.film_buckets() == 0
    r.set_film_buckets(8)
    r.launch("pt", 0)
    r.launch("light trace", 7)
    r.build_sampler()
    _fails(pkg, lambda: r.launch_eye_batch([1]), STATE, "buckets")
    r.set_film_moments(True)
    r.launch("pt", 1)
    _fails(pkg, lambda: r.adaptive_begin(2), STATE, "buckets")
    for s in (float("nan"), -0.5, 9.0):
        _fails(pkg, lambda: r.robust_resolve(s), INVALID, "strength")
    r.launch_deferred("pt", 2)
    _fails(pkg, r.robust_resolve, STATE, "deferred")
    r.merge_deferred(True)
    r.robust_resolve(8.0)
    # while adaptive sampling is active the switch cannot be turned on
    r.set_film_buckets(0)
    r.adaptive_begin(3)
    _fails(pkg, lambda: r.set_film_buckets(8), STATE, "adaptive")
    r.adaptive_end()
    # ... and with the buckets (and the moments) off the batched launch works again
    r.set_film_moments(False)
    r.launch("light trace", 9)
    r.build_sampler()
    r.launch_eye_batch([3])
    r.sync()
    assert np.isfinite(r.read_accum()).all()
