"""Geometry that cannot be built is refused before it reaches the BVH builder: spcbpt_create and spcbpt_create_lit answer
SPCBPT_ERR_INVALID_ARG, with a message that names the first offender, for a vertex coordinate, light corner or light edge that is NaN or
infinite and for a vertex index >= n_vertices -- and so do the .scene and glTF routes, which end in the same call.  The check runs before a
device is asked for, so all of this is tested without one (and no non-finite geometry is ever traced on a GPU)."""
import copy
import os

import numpy as np
import pytest

ERR_INVALID_ARG = -1


def _refused(pkg, scene):
    with pytest.raises(pkg.SpcbptError) as e:
        pkg.Renderer(scene, 0)
    assert f"({ERR_INVALID_ARG})" in str(e.value), str(e.value)
    return str(e.value)


def _cornell(pkg, lit=False):
    s = copy.deepcopy(pkg.scenes.cornell_box())
    s.vertices = np.array(s.vertices, dtype=np.float32)
    s.indices = np.array(s.indices, dtype=np.uint32)
    if lit:
        s.mesh_lights = [dict(material=1, emission=(1.0, 1.0, 1.0), n_patches=2)]   # spcbpt_create_lit
    return s


@pytest.mark.parametrize("lit", [False, True], ids=["create", "create_lit"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_vertex_is_refused_by_name(pkg, hip_lib, lit, bad):
    s = _cornell(pkg, lit)
    s.vertices[17, 1] = bad
    s.vertices[23, 0] = bad
    msg = _refused(pkg, s)
    assert "vertex 17 " in msg and "non-finite" in msg and "(y)" in msg, msg


@pytest.mark.parametrize("lit", [False, True], ids=["create", "create_lit"])
@pytest.mark.parametrize("field,bad", [("position", np.nan), ("position", np.inf), ("u", np.nan), ("u", -np.inf), ("v", np.nan), ("v", np.inf)])
def test_a_non_finite_light_is_refused(pkg, hip_lib, lit, field, bad):
    s = _cornell(pkg, lit)
    x = list(s.lights[0][field])
    x[2] = bad
    s.lights[0][field] = tuple(x)
    msg = _refused(pkg, s)
    assert "quad light 0 " in msg and "non-finite" in msg and "(z)" in msg, msg


def test_a_light_whose_corner_overflows_is_refused(pkg, hip_lib):
    s = _cornell(pkg)
    s.lights[0]["position"] = (3e38, 1.998, -0.25)
    s.lights[0]["u"] = (3e38, 0.0, 0.0)          # finite, but position + u is not
    msg = _refused(pkg, s)
    assert "quad light 0 " in msg and "(x)" in msg, msg


@pytest.mark.parametrize("lit", [False, True], ids=["create", "create_lit"])
def test_an_index_past_the_vertices_is_refused(pkg, hip_lib, lit):
    import ctypes as C
    s = _cornell(pkg, lit)
    n = len(s.vertices)
    sd, keep = s.desc()            # (Scene.desc checks the indices itself: the bad one goes into the array the C API is handed)
    C.cast(sd.indices, C.POINTER(C.c_uint32))[3 * 5 + 2] = n
    h = C.c_void_p()
    if lit:
        rc = hip_lib.spcbpt_create_lit(C.byref(sd), s.mesh_light_array(), len(s.mesh_lights), 0, C.byref(h))
    else:
        rc = hip_lib.spcbpt_create(C.byref(sd), 0, C.byref(h))
    msg = (hip_lib.spcbpt_last_error(None) or b"").decode()
    assert rc == ERR_INVALID_ARG and not h.value, (rc, msg)
    assert "vertex index out of range" in msg and "triangle 5" in msg and str(n) in msg, msg


def test_the_scene_file_route_refuses_an_infinite_vertex(pkg, hip_lib, tmp_path):
    """a coordinate of 1e39 in an OBJ of a .scene file: float32 has no such number"""
    s = _cornell(pkg)
    path = pkg.scenes.write_scene(s, str(tmp_path), "bad")
    obj = os.path.join(str(tmp_path), "bad", "mesh0.obj")
    lines = open(obj).read().splitlines()
    k = next(i for i, l in enumerate(lines) if l.startswith("v "))
    lines[k] = "v 1e39 0 1"
    open(obj, "w").write("\n".join(lines) + "\n")
    with pytest.raises(pkg.SpcbptError) as e:   # by the loader, or by spcbpt_create on what the loader hands over
        scene, _ = pkg.api.load_scene_file(path, str(tmp_path))
        pkg.Renderer(scene, 0)
    assert "no HIP device" not in str(e.value), str(e.value)


def test_the_gltf_route_refuses_a_nan_vertex(pkg, hip_lib, tmp_path):
    s = _cornell(pkg)
    path = pkg.scenes.write_gltf(s, str(tmp_path), "bad")
    blob_path = os.path.join(str(tmp_path), "bad.bin")
    blob = bytearray(open(blob_path, "rb").read())
    needle = s.vertices[s.indices[s.tri_material == 0].min()].tobytes()
    at = bytes(blob).find(needle)
    assert at >= 0
    blob[at + 4:at + 8] = np.float32(np.nan).tobytes()
    open(blob_path, "wb").write(bytes(blob))
    with pytest.raises(pkg.SpcbptError) as e:
        scene, _ = pkg.api.load_gltf(path)
        pkg.Renderer(scene, 0)
    assert "no HIP device" not in str(e.value), str(e.value)
