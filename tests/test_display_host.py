"""The display transform on the host -- the per-pixel code the kernels run (csrc/display_pixel.h) behind spcbpt_display_host -- against
the float64 numpy definition of tests/display_ref.py, on synthetic images.  Needs no GPU.

Bars.
  histogram  integer for integer: the bins are cut from the float32 luminance's bit pattern, the definition forms that luminance in
             float32 in the header's order, and nothing is rounded after it.
  EV         within 1e-5 of the float64 definition.  Derived: |EV| <= 32, so the one float32 rounding of the result is <= 2e-6; the
             eight bin-centre constants carry >= 9 digits; the sums are double on both sides.
  RGBA8      the byte is min(floor(code), 255) of the float64 codes, +-1 where the float64 code lies within 1e-3 of an integer in
             1 .. 255 (the tie rule of test_gpu_film_buckets.py: float32 may land on either side); at most 2 % of an image's channel
             values may sit at such a tie (2 values for the 7 x 5 and the 1 x 1 image), which the test asserts of the float64 reference first.
             Derived: ~10 float32 roundings of 6e-8 ahead of the quantisation are <= 6e-7 relative, 1.6e-4 of a code at 255.  Under
             auto exposure the codes are taken at the EV the call returned (a float32, held to the EV bar above by its own test):
             the definition's c' = c 2^EV reads the EV the pass applies.
Only finite pixels are judged for RGBA8; alpha is 255 everywhere."""
import ctypes as C

import numpy as np
import pytest

from tests import display_ref as ref
from tests.denoise_ref import tone_map_codes

INVALID = -1
EV_BAR = 1e-5
IDS = [f"{w}x{h}" for w, h in ref.SIZES] + ["edges"]


@pytest.fixture(scope="module")
def images():
    out = {f"{w}x{h}": ref.seeded_image(w, h) for w, h in ref.SIZES}
    out["edges"] = ref.edges_image()[0]
    return out


# ------------------------------------------------------------------------------------------------------------ histogram
@pytest.mark.parametrize("name", IDS)
def test_histogram_equals_the_definition(pkg, images, name):
    img = images[name]
    _, hist, _ = pkg.api.display_host(img)
    want = ref.histogram(img)
    assert hist.dtype == np.uint32 and hist.shape == (ref.COUNTERS,)
    assert int(hist.astype(np.int64).sum()) == img.shape[0] * img.shape[1]
    assert hist.tolist() == want.tolist()
    if name != "edges":
        assert hist[ref.DARK] == 0 and hist[ref.BRIGHT] == 0


def test_edges_image_counters(pkg):
    img, n, expected = ref.edges_image()
    # the hand-built pixels alone: each in the counter it was built for
    special = img.reshape(-1, 4)[:n]
    _, hist, _ = pkg.api.display_host(special)
    want = np.bincount(expected, minlength=ref.COUNTERS)
    assert hist.tolist() == want.tolist()
    assert ref.bins_of(ref.luminance32(special)).tolist() == expected
    for (edge, b), k in zip(ref.EDGE_BINS, range(9, n, 2)):
        assert expected[k] == b and expected[k + 1] == b - 1
    # the whole image: the rest is in range, so the two outer counters hold the hand-built pixels only -- zero, two negatives, NaN and
    # the predecessor of 2^-16 are dark; +inf and 2^16 are bright
    _, full, _ = pkg.api.display_host(img)
    assert int(full[ref.DARK]) == 5 and int(full[ref.BRIGHT]) == 2
    assert int(full.astype(np.int64).sum()) == 256
    assert int(full[0]) >= 1 and int(full[255]) >= 1


# ------------------------------------------------------------------------------------------------------------ EV
EV_CASES = {
    "defaults": dict(),
    "fractions 0 / 0": dict(low_fraction=0.0, high_fraction=0.0),
    "fractions 0.3 / 0.3": dict(low_fraction=0.3, high_fraction=0.3),
    "fractions 0.05 / 0.02, key 0.5, bias 1": dict(low_fraction=0.05, high_fraction=0.02, key=0.5, ev_bias=1.0),
    "clamped": None,   # a range that ends two stops below the image's free EV: built per image
}


@pytest.mark.parametrize("name", IDS)
@pytest.mark.parametrize("case", list(EV_CASES))
def test_auto_ev_matches_the_definition(pkg, images, name, case):
    img, params = images[name], EV_CASES[case]
    hist = ref.histogram(img)
    if case == "clamped":
        top = float(np.round(ref.auto_ev(hist))) - 2.0
        params = dict(ev_min=top - 1.5, ev_max=top)
    _, _, ev = pkg.api.display_host(img, auto=True, **params)
    want = ref.auto_ev(hist, **params)
    print(f"{name}, {case}: EV {ev:.7f}, definition {want:.7f}, |difference| {abs(ev - want):.2e} (bar {EV_BAR})")
    assert abs(ev - want) <= EV_BAR
    if case == "clamped":
        assert ev == params["ev_max"] == want                # to the bound exactly
    # with a previous EV and adapt 0.25 the EV moves a quarter of the way
    prev = 2.75
    _, _, ev2 = pkg.api.display_host(img, have_prev=True, prev_ev=prev, auto=True, adapt=0.25, **params)
    want2 = ref.auto_ev(hist, have_prev=True, prev_ev=prev, adapt=0.25, **params)
    assert abs(ev2 - want2) <= EV_BAR and abs(want2 - (prev + 0.25 * (want - prev))) <= 1e-12
    # adapt 1 forgets the previous EV; manual exposure ignores the state
    assert pkg.api.display_host(img, have_prev=True, prev_ev=prev, auto=True, **params)[2] == ev
    assert pkg.api.display_host(img, have_prev=True, prev_ev=prev, ev=1.5)[2] == 1.5


def test_no_in_range_pixel(pkg):
    img = np.zeros((4, 4, 4), np.float32)
    img[0, 0, :3] = 1e9
    assert pkg.api.display_host(img, auto=True, ev_bias=2.0)[2] == 2.0
    assert pkg.api.display_host(img, auto=True, ev_bias=20.0)[2] == 16.0
    assert pkg.api.display_host(img, have_prev=True, prev_ev=-3.25, auto=True, ev_bias=2.0, adapt=0.5)[2] == -3.25
    assert ref.auto_ev(ref.histogram(img), ev_bias=20.0) == 16.0


@pytest.mark.parametrize("name", IDS[:4])
@pytest.mark.parametrize("k", [-3, 5])
def test_scaling_by_a_power_of_two_shifts_bins_and_ev(pkg, images, name, k):
    img = images[name]
    scaled = img.copy()
    scaled[..., :3] *= np.float32(2.0 ** k)
    _, h0, ev0 = pkg.api.display_host(img, auto=True)
    _, h1, ev1 = pkg.api.display_host(scaled, auto=True)
    assert h0[ref.DARK] == h1[ref.DARK] == 0 and h0[ref.BRIGHT] == h1[ref.BRIGHT] == 0   # the result stays in range
    shifted = np.zeros(ref.BINS, np.uint32)
    if k > 0:
        shifted[8 * k:] = h0[:ref.BINS - 8 * k]
        assert not h0[ref.BINS - 8 * k:ref.BINS].any()
    else:
        shifted[:ref.BINS + 8 * k] = h0[-8 * k:ref.BINS]
        assert not h0[:-8 * k].any()
    assert h1[:ref.BINS].tolist() == shifted.tolist()
    assert abs(ev0) < 15 and abs(ev1) < 15                 # nothing clamps
    assert abs((ev1 - ev0) + k) <= EV_BAR


# ------------------------------------------------------------------------------------------------------------ RGBA8
EXPOSURES = [("ev -2", dict(ev=-2.0)), ("ev 0", dict(ev=0.0)), ("ev 3", dict(ev=3.0)), ("auto", dict(auto=True))]


@pytest.mark.parametrize("name", IDS)
@pytest.mark.parametrize("op", ref.OPS)
def test_bytes_match_the_float64_codes(pkg, images, name, op):
    img = images[name]
    finite = ref.finite_pixels(img)
    for label, how in EXPOSURES:
        out8, _, ev = pkg.api.display_host(img, op=op, **how)
        if "ev" in how:
            assert ev == how["ev"]
        else:
            assert abs(ev - ref.auto_ev(ref.histogram(img))) <= EV_BAR
        codes = ref.tone_codes(img, ev, op)
        # the float64 reference itself stays under the cap on this input
        assert int(ref.tie_mask(codes[finite]).sum()) <= ref.tie_cap(codes[finite].size)
        ties, differ = ref.check_bytes(out8, codes, finite)
        print(f"{name}, {op}, {label} (EV {ev:.4f}): {ties} of {codes[finite].size} values at a tie (cap {ref.tie_cap(codes[finite].size)}), {differ} differ by 1")
        assert out8.shape == img.shape
        if name != "1x1" and op != "linear":
            assert len(np.unique(out8[..., :3])) > (8 if name == "7x5" else 32)   # an image, not a constant


def test_white_sets_reinhards_shoulder(pkg, images):
    img = images["48x32"]
    for white in (1.0, 4.0, 50.0):
        out8, _, _ = pkg.api.display_host(img, op="reinhard", ev=1.0, white=white)
        ref.check_bytes(out8, ref.tone_codes(img, 1.0, "reinhard", white), ref.finite_pixels(img))
    lo = pkg.api.display_host(img, op="reinhard", ev=1.0, white=1.0)[0].astype(np.int64)
    hi = pkg.api.display_host(img, op="reinhard", ev=1.0, white=50.0)[0].astype(np.int64)
    assert (lo >= hi).all() and (lo > hi).any()


@pytest.mark.parametrize("name", IDS)
def test_default_operator_is_the_films_tone_map(pkg, images, name):
    img = images[name]
    finite = ref.finite_pixels(img)
    out8, _, ev = pkg.api.display_host(img)       # op 0, EV 0, manual
    assert ev == 0.0
    with np.errstate(all="ignore"):
        codes = tone_map_codes(img[..., :3])
    ref.check_bytes(out8, codes, finite)


# ------------------------------------------------------------------------------------------------------------ ABI
def test_params_struct_and_defaults(pkg, hip_lib):
    assert hip_lib.spcbpt_display_params_struct_size() == C.sizeof(pkg.api.DisplayParams) == 44
    sizes = (C.c_int32 * 32)()
    assert hip_lib.spcbpt_abi_struct_sizes(sizes, 32) == 13                   # no new entry
    p = pkg.api.DisplayParams()
    assert hip_lib.spcbpt_display_default_params(C.byref(p)) == 0
    got = [getattr(p, n) for n, _ in pkg.api.DisplayParams._fields_]
    want = [0, 0, 0.0, 0.18, 0.05, 0.02, 0.0, -16.0, 16.0, 1.0, 4.0]
    assert got == [np.float32(v) if isinstance(v, float) else v for v in want]
    assert hip_lib.spcbpt_display_default_params(None) == INVALID


def _host_rc(pkg, hip_lib, img, p, n=None):
    x = np.ascontiguousarray(img, np.float32)
    out = np.zeros(x.shape, np.uint8)
    return hip_lib.spcbpt_display_host(x.ctypes.data_as(C.POINTER(C.c_float)), x.size // 4 if n is None else n, C.byref(p), 0, 0.0, out.ctypes.data, None, None)


def test_invalid_parameters_are_refused(pkg, hip_lib):
    img = ref.seeded_image(7, 5)
    ok = pkg.api.display_params
    assert _host_rc(pkg, hip_lib, img, ok()) == 0
    bad = [dict(op=-1), dict(op=4), dict(flags=4), dict(low_fraction=-0.1), dict(low_fraction=1.0), dict(high_fraction=1.0), dict(high_fraction=-0.01),
           dict(low_fraction=0.5, high_fraction=0.5), dict(low_fraction=0.7, high_fraction=0.4), dict(ev_min=1.0, ev_max=0.0),
           dict(adapt=0.0), dict(adapt=-0.5), dict(adapt=1.5), dict(key=0.0), dict(key=-1.0), dict(white=0.0)]
    for field in ("ev", "key", "low_fraction", "high_fraction", "ev_bias", "ev_min", "ev_max", "adapt", "white"):
        bad += [{field: float("nan")}, {field: float("inf")}, {field: float("-inf")}]
    for kw in bad:
        for auto in (False, True):
            assert _host_rc(pkg, hip_lib, img, ok(auto=auto, **kw)) == INVALID, kw
        with pytest.raises(pkg.SpcbptError) as e:
            pkg.api.display_host(img, **kw)
        assert "(-1)" in str(e.value)
    assert _host_rc(pkg, hip_lib, img, ok(low_fraction=0.5, high_fraction=0.49, adapt=1.0, ev_min=2.0, ev_max=2.0)) == 0
    for n in (-1, 0, (1 << 28) + 1):
        assert _host_rc(pkg, hip_lib, img, ok(), n) == INVALID
    fp = C.POINTER(C.c_float)
    assert hip_lib.spcbpt_display_host(None, 35, C.byref(ok()), 0, 0.0, None, None, None) == INVALID
    assert hip_lib.spcbpt_display_host(img.ctypes.data_as(fp), 35, None, 0, 0.0, None, None, None) == INVALID
    assert hip_lib.spcbpt_display_host(img.ctypes.data_as(fp), 35, C.byref(ok()), 0, 0.0, None, None, None) == 0   # every output is optional
    with pytest.raises(pkg.SpcbptError):
        pkg.api.display_params(gamma=2.2)
