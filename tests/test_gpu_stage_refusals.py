"""What the image-space stages refuse, message by message: spcbpt_display / spcbpt_bloom / spcbpt_local_tone and their *_image forms, the
three denoisers (spcbpt_denoise, spcbpt_denoise_variance, spcbpt_history_denoise) and the three plane readers.  Every expected text is
written out whole here, so that the stages' shared plumbing (Context::linear_image, Context::caller_image, Context::denoise_begin) cannot
change a word of what one of them says, nor the order in which its checks apply, without this file failing."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_mesh_light import _renderer

pytestmark = pytest.mark.gpu

STATE, INVALID = -5, -1
FILM, DENOISED, ROBUST, HISTORY, BLOOM, LOCAL = range(6)
STAGES = ("display", "bloom", "local_tone")
LAST_SOURCE = dict(display=LOCAL, bloom=HISTORY, local_tone=BLOOM)

RANGE = dict(display="display: source must be 0 (film), 1 (denoised), 2 (robust), 3 (history), 4 (bloom) or 5 (local)",
             bloom="bloom: source must be 0 (film), 1 (denoised), 2 (robust) or 3 (history)",
             local_tone="local_tone: source must be 0 (film), 1 (denoised), 2 (robust), 3 (history) or 4 (bloom)")
DEFERRED = "a deferred frame is outstanding: spcbpt_merge_deferred(ctx, keep) first"
NO_DENOISED = "no denoised image: spcbpt_denoise / spcbpt_denoise_variance / spcbpt_history_denoise since the last spcbpt_resize"
BUCKETS_OFF = "no robust image: the film's buckets are off (spcbpt_set_film_buckets, then spcbpt_robust_resolve)"
NO_RESOLVE = "no robust image: no spcbpt_robust_resolve since the film's buckets were last set up"
NO_HISTORY = "no resolved history image: spcbpt_history_resolve since the last spcbpt_resize / spcbpt_history_reset"
NO_BLOOM = "no bloom plane: spcbpt_bloom / spcbpt_bloom_image since the last spcbpt_resize"
NO_LOCAL = "no local tone plane: spcbpt_local_tone / spcbpt_local_tone_image since the last spcbpt_resize"
READ = dict(read_display="read_display: no spcbpt_display / spcbpt_display_image since the last spcbpt_resize",
            read_bloom="read_bloom: no spcbpt_bloom / spcbpt_bloom_image since the last spcbpt_resize",
            read_local_tone="read_local_tone: no spcbpt_local_tone / spcbpt_local_tone_image since the last spcbpt_resize")
DENOISERS = ("denoise", "denoise_variance", "history_denoise")
NEEDS_FEATURES = " needs the feature buffers: spcbpt_launch_features since the last spcbpt_resize"


def _refuses(pkg, fn, code, text):
    """The call raises, with `code` and with `text` as the whole of the library's message."""
    with pytest.raises(pkg.SpcbptError) as e:
        fn()
    assert str(e.value).endswith(f" failed ({code}): {text}"), str(e.value)


def _box(pkg):
    return _renderer(pkg, pkg.scenes.cornell_box(), 48, 32)


def test_source_range(gpu, pkg):
    r = _box(pkg)
    for stage in STAGES:
        for source in (-1, LAST_SOURCE[stage] + 1, 7):
            _refuses(pkg, lambda: getattr(r, stage)(source), INVALID, RANGE[stage])
    r.launch("pt", 0)
    r.launch_deferred("pt", 1)                                 # the range comes before the state
    for stage in STAGES:
        _refuses(pkg, lambda: getattr(r, stage)(-1), INVALID, RANGE[stage])
    r.merge_deferred(True)


def test_a_deferred_frame(gpu, pkg):
    r = _box(pkg)
    r.bloom_image(np.ones((3, 2, 4), np.float32))
    r.launch("pt", 0)
    r.launch_deferred("pt", 1)
    for stage in STAGES:
        for source in range(LAST_SOURCE[stage] + 1):           # ... before any word about the source's plane, present (film, bloom) or not
            _refuses(pkg, lambda: getattr(r, stage)(source), STATE, f"{stage}: {DEFERRED}")
    r.merge_deferred(True)
    for stage in STAGES:
        getattr(r, stage)("film")


def test_missing_planes(gpu, pkg):
    r = _box(pkg)
    r.launch("pt", 0)
    for stage in STAGES:
        _refuses(pkg, lambda: getattr(r, stage)("denoised"), STATE, f"{stage}: {NO_DENOISED}")
        _refuses(pkg, lambda: getattr(r, stage)("robust"), STATE, f"{stage}: {BUCKETS_OFF}")
        _refuses(pkg, lambda: getattr(r, stage)("history"), STATE, f"{stage}: {NO_HISTORY}")
    r.set_film_buckets(4)
    for stage in STAGES:
        _refuses(pkg, lambda: getattr(r, stage)("robust"), STATE, f"{stage}: {NO_RESOLVE}")
    r.set_film_buckets(0)
    _refuses(pkg, lambda: r.display("bloom"), STATE, f"display: {NO_BLOOM}")
    _refuses(pkg, lambda: r.local_tone("bloom"), STATE, f"local_tone: {NO_BLOOM}")
    _refuses(pkg, lambda: r.display("local"), STATE, f"display: {NO_LOCAL}")
    for name in READ:                                          # the refused calls left nothing behind
        _refuses(pkg, getattr(r, name), STATE, READ[name])


def test_a_context_that_was_never_resized(gpu, pkg):
    r = pkg.Renderer(pkg.scenes.cornell_box(), 0)
    for stage in STAGES:
        for source in (FILM, DENOISED, ROBUST, HISTORY):       # the film-sized sources: the film's absence is said before the plane's
            _refuses(pkg, lambda: getattr(r, stage)(source), STATE, f"{stage} before spcbpt_resize")
    _refuses(pkg, lambda: r.display("bloom"), STATE, f"display: {NO_BLOOM}")     # the planes of a size of their own need no film
    _refuses(pkg, lambda: r.local_tone("bloom"), STATE, f"local_tone: {NO_BLOOM}")
    _refuses(pkg, lambda: r.display("local"), STATE, f"display: {NO_LOCAL}")
    for name in DENOISERS:
        _refuses(pkg, getattr(r, name), STATE, f"{name} before spcbpt_resize")


def test_caller_images(gpu, pkg):
    """The size check comes before anything reads the image, so a small buffer under a shape claim of 2^28 + 1 pixels is safe."""
    r = _box(pkg)
    small = np.ones((2, 2, 4), np.float32)
    ptr = small.ctypes.data_as(C.POINTER(C.c_float))
    params = dict(display=pkg.api.display_params(), bloom=pkg.api.bloom_params(), local_tone=pkg.api.local_tone_params())
    for stage in STAGES:
        fn, p = getattr(r.lib, f"spcbpt_{stage}_image"), params[stage]
        for w, h in (((1 << 28) + 1, 1), (1, (1 << 28) + 1), (1 << 14, (1 << 14) + 1), (0, 4), (4, 0), (-2, 2), (1 << 16, 1 << 16)):
            _refuses(pkg, lambda: r._chk(fn(r.h, ptr, w, h, C.byref(p)), stage), INVALID, f"{stage}_image: the image must hold 1 .. 2^28 pixels")
        _refuses(pkg, lambda: r._chk(fn(r.h, None, 2, 2, C.byref(p)), stage), INVALID, "null pointer")
        _refuses(pkg, lambda: r._chk(fn(r.h, None, 0, 0, C.byref(p)), stage), INVALID, "null pointer")   # the null check is the first of the two
        _refuses(pkg, lambda: r._chk(fn(r.h, ptr, 2, 2, None), stage), INVALID, "null params")
    for name in READ:                                          # the refused calls left nothing behind
        _refuses(pkg, getattr(r, name), STATE, READ[name])
    for stage in STAGES:
        getattr(r, f"{stage}_image")(small)
    assert r.read_display()[0].shape == r.read_bloom().shape == r.read_local_tone().shape == (2, 2, 4)


def test_denoisers(gpu, pkg):
    r = _box(pkg)
    _refuses(pkg, r.denoise, STATE, "denoise" + NEEDS_FEATURES)
    _refuses(pkg, r.history_denoise, STATE, "history_denoise" + NEEDS_FEATURES)
    _refuses(pkg, r.denoise_variance, STATE, "denoise_variance needs the film's moments: spcbpt_set_film_moments(ctx, 1) before the frames are rendered")
    r.set_film_moments(True)
    _refuses(pkg, r.denoise_variance, STATE, "denoise_variance" + NEEDS_FEATURES)
    r.launch("pt", 0)
    r.launch_features(0)
    _refuses(pkg, r.history_denoise, STATE, "history_denoise needs a resolved image: spcbpt_history_resolve since the last spcbpt_resize / spcbpt_history_reset")
    r.set_film_moments(False)
    r.history_resolve(1)
    _refuses(pkg, r.history_denoise, STATE, "history_denoise: the resolved image has no variance -- the moments were off at the capture or resolve "
                                            "(spcbpt_set_film_moments(ctx, 1) before both)")
    r.set_film_moments(True)
    r.launch("pt", 1)
    r.history_resolve(2)
    nan = float("nan")
    for name in DENOISERS:                                     # every precondition holds now: the parameters are looked at
        fn = getattr(r, name)
        for it in (0, 9, -1):
            _refuses(pkg, lambda: fn(iterations=it), INVALID, f"{name}: iterations must be in 1..8")
        for k in range(1, 4):
            args = [5, 0.0, 0.0, 0.0]
            args[k] = nan
            _refuses(pkg, lambda: fn(*args), INVALID, f"{name}: a sigma is not a number")
        _refuses(pkg, lambda: fn(0, nan), INVALID, f"{name}: iterations must be in 1..8")   # the iterations first
    _refuses(pkg, r.read_denoised, STATE, "read_denoised: no spcbpt_denoise since the last spcbpt_resize")
    r.launch_deferred("pt", 2)
    for name in DENOISERS:                                     # no prefix, and ahead of the parameters
        _refuses(pkg, getattr(r, name), STATE, DEFERRED)
        _refuses(pkg, lambda: getattr(r, name)(iterations=0), STATE, DEFERRED)
    r.merge_deferred(True)
    for name in DENOISERS:
        getattr(r, name)(iterations=1)
        assert r.read_denoised()[0].shape == (32, 48, 4)


def test_readers(gpu, pkg):
    r = _box(pkg)
    for name in READ:
        _refuses(pkg, getattr(r, name), STATE, READ[name])
    _refuses(pkg, r.read_display_histogram, STATE, READ["read_display"])
    img = np.ones((5, 7, 4), np.float32)
    r.display_image(img, ev=1.0)
    r.bloom_image(img)
    r.local_tone_image(img)
    assert r.read_display()[0].shape == r.read_bloom().shape == r.read_local_tone().shape == (5, 7, 4)
    _refuses(pkg, r.read_display_histogram, STATE, "read_display: the last display call computed no histogram (manual exposure without SPCBPT_DISPLAY_HISTOGRAM)")
    r.resize(48, 32)
    for name in READ:
        _refuses(pkg, getattr(r, name), STATE, READ[name])
