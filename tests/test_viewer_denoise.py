"""The viewer's denoise switch (spcbpt_viewer_set_denoise / spcbpt_viewer_get_denoise) on a null context: state only there -- it needs
the reproject switch, falls with it, and flipping it restarts the accumulation.  Needs no GPU; what the switch does on a context is
tests/test_gpu_history_denoise.py."""
import ctypes as C

import pytest

from tests.viewer_scripts import scripts


def _viewer(pkg, s, w=96, h=64):
    return pkg.api.Viewer(None, s["eye"], s["lookat"], s["up"], float(s["fov"]), w, h)


def test_switch_needs_reproject_and_falls_with_it(hip_lib, pkg):
    v = _viewer(pkg, scripts()[0])
    assert v.get_denoise() is False                               # off by default
    with pytest.raises(pkg.SpcbptError, match=r"\(-5\)"):
        v.set_denoise(True)                                       # it filters the resolved image: not without reproject
    assert v.get_denoise() is False
    v.set_denoise(False)                                          # no flip: fine without reproject
    v.set_reproject(True)
    v.set_denoise(True)
    assert v.get_denoise() is True and v.get_reproject() == {"on": 1, "live": 0}
    v.set_reproject(False)
    assert v.get_denoise() is False and v.get_reproject() == {"on": 0, "live": 0}
    on = C.c_int32(7)
    assert hip_lib.spcbpt_viewer_set_denoise(None, 1) == -1 and hip_lib.spcbpt_viewer_get_denoise(None, C.byref(on)) == -1
    assert hip_lib.spcbpt_viewer_get_denoise(v.h, None) == -1
    assert hip_lib.spcbpt_viewer_get_denoise(v.h, C.byref(on)) == 0 and on.value == 0


def test_flipping_the_switch_restarts_the_accumulation(hip_lib, pkg):
    v = _viewer(pkg, scripts()[1])
    v.set_reproject(True)
    for _ in range(3):
        v.frame()
    assert v.state()["subframe_index"] == 3
    v.set_denoise(True); v.frame()
    assert v.state()["subframe_index"] == 1                       # the frame after the flip was subframe 0
    v.set_denoise(True); v.frame()                                # no flip: the accumulation goes on
    assert v.state()["subframe_index"] == 2
    v.set_denoise(False); v.frame()
    assert v.state()["subframe_index"] == 1
