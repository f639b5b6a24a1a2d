"""The batched film merge with moments and buckets on the host -- the per-pixel function k_film_merge_batch_stats runs
(csrc/merge_stats_pixel.h) behind spcbpt_film_merge_batch_host -- against the sequential application, frame by frame, of
spcbpt_film_moments_update_host, spcbpt_film_buckets_update_host (which zeroes every bucket at subframe 0) and a float32 numpy
`c + a * (x - c)`.  Bit for bit: every comparison is on the arrays' bytes.  Needs no GPU."""
import numpy as np
import pytest

INVALID = -1


def _samples(rng, n, pixels):
    """(n, pixels, 4) float32: random samples with exact zeros and huge values among them (no NaN, no infinity: the film holds none)."""
    x = rng.random((n, pixels, 4), dtype=np.float32) * np.float32(4.0)
    x[rng.random((n, pixels)) < 0.15] = 0.0
    huge = rng.random((n, pixels)) < 0.1
    x[huge] *= np.float32(1e17)   # (squares of differences stay finite in M2: 32 x (4e17)^2 = 5e36)
    x[..., 3] = 1.0
    return x


def _sequential(api, x, subframes, accum, m2n, planes):
    """Frame by frame: the moments update from the mean before the merge, the bucket update, the mean's update in float32."""
    c = accum.copy()
    for k, sf in enumerate(subframes):
        if m2n is not None:
            api.film_moments_update_host(c, x[k], sf, m2n)
        if planes is not None:
            api.film_buckets_update_host(x[k], sf, planes)
        if sf == 0:
            c = x[k].copy()
        else:
            a = np.float32(1.0) / np.float32(sf + 1)
            c[..., :3] = c[..., :3] + a * (x[k][..., :3] - c[..., :3])
        assert c.dtype == np.float32
        c[..., 3] = 1.0
    return c


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _lists(n):
    yield list(range(n))
    yield list(range(5, 5 + n))


CASES = [(n, sf) for n in (1, 5, 32) for sf in _lists(n)] + [(5, [3, 4, 0, 1, 2]), (3, [2, 4, 9])]


@pytest.mark.parametrize("pixels", [1, 2, 3, 200])
@pytest.mark.parametrize("K", [0, 3, 7, 32])
@pytest.mark.parametrize("moments", [False, True])
def test_batch_equals_the_sequential_updates(hip_lib, pkg, pixels, K, moments):
    api = pkg.api
    rng = np.random.default_rng(1000 * pixels + 10 * K + int(moments))
    for n, subframes in CASES:
        x = _samples(rng, n, pixels)
        for fresh in (False, True):   # fresh: zeroed planes in front of subframes > 0 -- the switches turned on in mid-film
            accum = _samples(rng, 1, pixels)[0]
            m2n = planes = None
            if moments:
                m2n = np.zeros((pixels, 4), np.float32)
                if not fresh:
                    m2n[:, :3] = rng.random((pixels, 3), dtype=np.float32) * np.float32(10.0)
                    m2n[:, 3] = np.float32(subframes[0])
            if K:
                planes = np.zeros((K, pixels, 4), np.float32)
                if not fresh:
                    planes[...] = _samples(rng, K, pixels)
                    planes[..., 3] = rng.integers(0, 9, (K, pixels)).astype(np.float32)
            want_m, want_p = (None if m2n is None else m2n.copy()), (None if planes is None else planes.copy())
            want_c = _sequential(api, x, subframes, accum, want_m, want_p)
            got = api.film_merge_batch_host(x, subframes, accum, m2n, planes)
            assert got is accum
            tag = (n, subframes, fresh)
            assert _same(accum, want_c), tag
            if moments:
                assert _same(m2n, want_m), tag
            if K:
                assert _same(planes, want_p), tag


def test_zeroed_moments_with_later_subframes_count_the_merges_since(hip_lib, pkg):
    """The switch turned on in mid-film: a zeroed m2n in front of subframes 3, 4, 5 -- n counts the merges since, M2 is their sum."""
    api = pkg.api
    rng = np.random.default_rng(7)
    x = _samples(rng, 3, 50)
    accum = _samples(rng, 1, 50)[0]
    m2n = np.zeros((50, 4), np.float32)
    want_m = m2n.copy()
    want_c = _sequential(api, x, [3, 4, 5], accum, want_m, None)
    api.film_merge_batch_host(x, [3, 4, 5], accum, m2n, None)
    assert _same(m2n, want_m) and _same(accum, want_c)
    assert (m2n[:, 3] == 3.0).all()


def test_bad_arguments(hip_lib, pkg):
    import ctypes as C
    f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    x = np.zeros((2, 4, 4), np.float32)
    a = np.zeros((4, 4), np.float32)
    p = np.zeros((3, 4, 4), np.float32)
    sf = np.array([0, 1], np.uint32)
    fp = lambda v: v.ctypes.data_as(f32p)
    call = hip_lib.spcbpt_film_merge_batch_host
    assert call(fp(x), sf.ctypes.data_as(u32p), 2, 4, 3, fp(a), None, fp(p)) == 0
    assert call(None, sf.ctypes.data_as(u32p), 2, 4, 0, fp(a), None, None) == INVALID
    assert call(fp(x), None, 2, 4, 0, fp(a), None, None) == INVALID
    assert call(fp(x), sf.ctypes.data_as(u32p), 2, 4, 0, None, None, None) == INVALID
    assert call(fp(x), sf.ctypes.data_as(u32p), 0, 4, 0, fp(a), None, None) == INVALID
    assert call(fp(x), sf.ctypes.data_as(u32p), 33, 4, 0, fp(a), None, None) == INVALID
    assert call(fp(x), sf.ctypes.data_as(u32p), 2, 0, 0, fp(a), None, None) == INVALID
    assert call(fp(x), sf.ctypes.data_as(u32p), 2, 4, 2, fp(a), None, fp(p)) == INVALID     # K outside 3 .. 32
    assert call(fp(x), sf.ctypes.data_as(u32p), 2, 4, 33, fp(a), None, fp(p)) == INVALID
    assert call(fp(x), sf.ctypes.data_as(u32p), 2, 4, 3, fp(a), None, None) == INVALID      # buckets without planes
