"""The one staging buffer behind spcbpt_display_image, spcbpt_bloom_image and spcbpt_local_tone_image (Context::image_link): calls of the
three stages queued back to back, with images of growing and shrinking size and no read in between, each see their own image -- the
upload of the next call is queued behind the kernels of the previous one, and a buffer that has to grow is freed only after they ran.
The planes are held to the host forms as tests/test_gpu_bloom.py, tests/test_gpu_local_tone.py (bit for bit) and
tests/test_gpu_display.py (outside its quantisation ties) hold them."""
import pytest

from tests import bloom_ref, display_ref, local_tone_ref
from tests.test_gpu_display import _against_host
from tests.test_gpu_mesh_light import _renderer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu, pkg, hip_lib):
    assert hip_lib.spcbpt_build_arithmetic().decode() == "ieee"
    return _renderer(pkg, pkg.scenes.cornell_box(), 48, 32)


def test_back_to_back_calls_each_see_their_own_image(pkg, ctx):
    r = ctx
    a, b, c = display_ref.seeded_image(7, 5), bloom_ref.seeded_image(48, 32), local_tone_ref.seeded_image(9, 6)
    r.display_image(a, op="aces", ev=1.0)
    r.bloom_image(b, strength=0.3)                             # the staging buffer grows ...
    r.local_tone_image(c, cell=4, compress=0.5, detail=1.2)    # ... and does not shrink
    r.display_image(b, op="reinhard", auto=True)
    assert r.read_bloom().tobytes() == pkg.api.bloom_host(b, strength=0.3).tobytes()
    assert r.read_local_tone().tobytes() == pkg.api.local_tone_host(c, cell=4, compress=0.5, detail=1.2).tobytes()
    _against_host(pkg, r, b, "staging: display_image(B) behind three other calls", op="reinhard", auto=True)


@pytest.mark.parametrize("freed", [False, True], ids=["grown", "freed"])
def test_a_larger_upload_behind_a_display_call_leaves_its_plane_alone(pkg, ctx, freed):
    """display_image(A), then a bloom_image whose image needs a larger staging buffer than any call before it, then the read: the display
    kernels ran on A, not on what the next upload wrote or on freed memory.  `freed`: the same after a resize has released the buffer."""
    r = ctx
    if freed:
        r.resize(48, 32)
    a = display_ref.seeded_image(7, 5, seed=1)
    b = bloom_ref.seeded_image(*((48, 32) if freed else (130, 67)), seed=2)
    r.display_reset()
    r.display_image(a, op="aces", auto=True)
    r.bloom_image(b)
    r.local_tone_image(a)
    _against_host(pkg, r, a, "staging: display_image(A) ahead of a larger bloom_image", op="aces", auto=True)
    assert r.read_bloom().tobytes() == pkg.api.bloom_host(b).tobytes()
    assert r.read_local_tone().tobytes() == pkg.api.local_tone_host(a).tobytes()
