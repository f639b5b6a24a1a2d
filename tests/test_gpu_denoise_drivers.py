"""The three denoisers (spcbpt_denoise, spcbpt_denoise_variance, spcbpt_history_denoise) share one driver -- Context::denoise_run: the
parameter check, the sigma defaults, the reservation of the five planes, the parameter record, the remodulate tail -- and one set of
planes.  Run one after the other on one context, in either order, each returns byte for byte what it returns on a context of its own
that never ran another: no state of one call reaches the next."""
import pytest

from tests.test_gpu_mesh_light import _renderer

pytestmark = pytest.mark.gpu

FRAMES = 4
# an even and an odd number of passes (the result leaves from the other of the two planes), defaults and sigmas of the caller's
CALLS = (("denoise", (4, 0.0, 0.0, 0.0)), ("denoise_variance", (5, 3.0, 0.5, 0.2)), ("history_denoise", (2, 0.0, 0.25, 0.0)))


def _context(pkg):
    """The Cornell box at 48 x 32 with the moments on: 4 frames of "pt", the features, a capture and a resolve."""
    r = _renderer(pkg, pkg.scenes.cornell_box(), 48, 32)
    r.set_film_moments(True)
    for f in range(FRAMES):
        r.launch("pt", f)
        r.launch_features(f)
    r.history_capture(FRAMES)
    r.history_resolve(FRAMES)
    return r


def _run(r, name, args):
    getattr(r, name)(*args)
    return tuple(a.tobytes() for a in r.read_denoised())       # the float4 plane and its RGBA8 frame


@pytest.fixture(scope="module")
def alone(gpu, pkg, hip_lib):
    """What each denoiser returns on a context that runs nothing else."""
    assert hip_lib.spcbpt_build_arithmetic().decode() == "ieee"
    out = {}
    for name, args in CALLS:
        r = _context(pkg)
        out[name] = _run(r, name, args)
        r.close()
    assert len(set(out.values())) == 3                         # three different images: the comparison below can tell them apart
    return out


def test_denoisers_on_one_context_are_the_denoisers_alone(pkg, alone):
    r = _context(pkg)
    for name, args in CALLS + CALLS[::-1]:
        assert _run(r, name, args) == alone[name], name
    r.close()
