"""The viewer's history-reprojection switch (spcbpt_viewer_set_reproject / spcbpt_viewer_get_reproject) on a null context: the switch is
state only there, no prior is ever live, and the subframe bookkeeping of a session is the same with and without it.  Needs no GPU;
what the switch does on a context is tests/test_gpu_reproject.py."""
import ctypes as C

from tests.viewer_scripts import scripts


def _viewer(pkg, s, w=96, h=64):
    return pkg.api.Viewer(None, s["eye"], s["lookat"], s["up"], float(s["fov"]), w, h)


def _session(v):
    """A session with every kind of restart; the subframe index the next frame will render, after every step."""
    out = []

    def show(n=1):
        for _ in range(n):
            v.frame()
            out.append((v.state()["subframe_index"], v.state()["alg"], v.state()["camera_changed"]))

    show(4)
    v.mouse_button("left", 1, 10, 10); v.cursor_pos(30, 18); v.mouse_button("left", 0, 30, 18)
    show(3)
    v.scroll(1); show(2)
    v.key("SPACE"); show(2)
    v.window_size(80, 48); show(2)
    v.key("P"); show(2)
    v.key("P"); show(2)
    v.mouse_button("right", 1, 10, 10); v.cursor_pos(12, 11); show(1); v.cursor_pos(14, 12); show(1); v.mouse_button("right", 0, 14, 12); show(2)
    return out


def test_switch_is_state_only_without_a_context(hip_lib, pkg):
    v = _viewer(pkg, scripts()[0])
    assert v.get_reproject() == {"on": 0, "live": 0}             # off by default
    v.set_reproject(True)
    assert v.get_reproject() == {"on": 1, "live": 0}
    for _ in range(3):
        v.frame()
    assert v.get_reproject() == {"on": 1, "live": 0}             # no move yet
    v.mouse_button("left", 1, 10, 10); v.cursor_pos(30, 18); v.mouse_button("left", 0, 30, 18)
    v.frame()
    assert v.get_reproject() == {"on": 1, "live": 0}             # nothing is launched without a context: nothing is live
    assert v.state()["subframe_index"] == 1
    v.set_reproject(False)
    assert v.get_reproject() == {"on": 0, "live": 0}
    # NULL arguments: the viewer is required, either output may be left out
    on = C.c_int32(7)
    assert hip_lib.spcbpt_viewer_set_reproject(None, 1) == -1 and hip_lib.spcbpt_viewer_get_reproject(None, C.byref(on), None) == -1
    assert hip_lib.spcbpt_viewer_get_reproject(v.h, None, None) == 0
    assert hip_lib.spcbpt_viewer_get_reproject(v.h, C.byref(on), None) == 0 and on.value == 0


def test_flipping_the_switch_restarts_the_accumulation(hip_lib, pkg):
    v = _viewer(pkg, scripts()[1])
    for _ in range(3):
        v.frame()
    assert v.state()["subframe_index"] == 3
    v.set_reproject(True); v.frame()
    assert v.state()["subframe_index"] == 1                       # the frame after the flip was subframe 0
    v.set_reproject(True); v.frame()                              # no flip: the accumulation goes on
    assert v.state()["subframe_index"] == 2
    v.set_reproject(False); v.frame()
    assert v.state()["subframe_index"] == 1


def test_subframe_bookkeeping_does_not_depend_on_the_switch(hip_lib, pkg):
    s = scripts()[2]
    plain, switched = _viewer(pkg, s), _viewer(pkg, s)
    switched.set_reproject(True)
    a, b = _session(plain), _session(switched)
    assert a == b and len(a) == 21
    assert switched.get_reproject() == {"on": 1, "live": 0} and plain.get_reproject() == {"on": 0, "live": 0}
    for k in ("eye", "lookat", "up", "U", "V", "W"):
        assert plain.state()[k].tobytes() == switched.state()[k].tobytes()
