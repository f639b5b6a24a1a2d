"""Mesh lights, the host side (no GPU): the glTF route (emissive materials -> spcbpt_scene_file_mesh_lights, next to and not inside the
scene desc) and the sampling table spcbpt_create_lit builds for a light (spcbpt_mesh_light_table: areas, CMF, Morton patches)
against numpy float64."""
import ctypes as C
import json
import os

import numpy as np
import pytest


def _two_lamp_scene(pkg):
    """simple_room plus two emissive meshes: an icosphere (material 3, emission above 1: needs the strength extension) and a
    tetrahedron (material 4, emission below 1)."""
    sc = pkg.scenes.simple_room()
    v1, f1 = pkg.scenes.icosphere((0.4, 1.4, 0.3), 0.15, 1)
    v2 = np.array([(-0.5, 1.2, 0.2), (-0.3, 1.25, 0.2), (-0.4, 1.2, 0.4), (-0.4, 1.45, 0.3)])
    f2 = np.array([(0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3)], np.uint32)
    nv = sc.vertices.shape[0]
    sc.vertices = np.concatenate([sc.vertices, v1.astype(np.float32), v2.astype(np.float32)])
    sc.texcoords = np.concatenate([sc.texcoords, np.zeros((len(v1) + len(v2), 2), np.float32)])
    sc.indices = np.concatenate([sc.indices, f1 + np.uint32(nv), f2 + np.uint32(nv + len(v1))])
    sc.tri_material = np.concatenate([sc.tri_material, np.full(len(f1), 3, np.int32), np.full(len(f2), 4, np.int32)])
    sc.materials += [dict(color=(1, 1, 1), roughness=1.0, metallic=0.0), dict(color=(1, 1, 1), roughness=1.0, metallic=0.0)]
    sc.mesh_lights = [dict(material=3, emission=(12.0, 9.0, 5.0), n_patches=6), dict(material=4, emission=(0.5, 0.75, 0.25), n_patches=6)]
    return sc


def _desc_bytes(lib, h, pkg):
    d = pkg.api.SceneDesc()
    assert lib.spcbpt_scene_file_desc(h, C.byref(d)) == 0
    grab = lambda p, n: C.string_at(p, n) if n else b""
    return (d.n_vertices, d.n_triangles, d.n_materials, d.n_textures, d.n_lights, grab(d.vertices, 12 * d.n_vertices),
            grab(d.texcoords, 8 * d.n_vertices), grab(d.indices, 12 * d.n_triangles), grab(d.tri_material, 4 * d.n_triangles),
            grab(C.cast(d.materials, C.c_void_p), C.sizeof(pkg.api.Material) * d.n_materials),
            grab(C.cast(d.lights, C.c_void_p), C.sizeof(pkg.api.QuadLight) * d.n_lights))


def test_mesh_light_struct_mirror(hip_lib, pkg):
    assert hip_lib.spcbpt_mesh_light_struct_size() == C.sizeof(pkg.api.MeshLight) == 20


def test_gltf_round_trip_of_emissive_materials(hip_lib, pkg, tmp_path):
    sc = _two_lamp_scene(pkg)
    path = pkg.scenes.write_gltf(sc, str(tmp_path), "lamps")
    doc = json.load(open(path))
    assert doc["materials"][3]["extensions"]["KHR_materials_emissive_strength"]["emissiveStrength"] == 16.0
    assert "extensions" not in doc["materials"][4] and doc["materials"][4]["emissiveFactor"] == [0.5, 0.75, 0.25]
    back, warn = pkg.load_gltf(path, emissive=True)
    assert [m["material"] for m in back.mesh_lights] == [3, 4]
    assert np.array_equal(np.array(back.mesh_lights[0]["emission"], np.float32), np.array([12, 9, 5], np.float32))
    assert np.array_equal(np.array(back.mesh_lights[1]["emission"], np.float32), np.array([0.5, 0.75, 0.25], np.float32))
    assert [m["n_patches"] for m in back.mesh_lights] == [6, 6]       # root extras.spcbpt_mesh_light_patches
    assert "emissive" not in warn and "doubleSided" not in warn
    # default: the emissive materials are ignored, as before
    plain, _ = pkg.load_gltf(path)
    assert plain.mesh_lights == [] and len(plain.lights) == 1

    # the desc does not depend on the emissive factors: the same file with every emissive key removed gives the same bytes
    for m in doc["materials"]:
        m.pop("emissiveFactor", None); m.pop("extensions", None)
    doc.pop("extensionsUsed", None); doc["extras"].pop("spcbpt_mesh_light_patches", None)
    bare = os.path.join(str(tmp_path), "bare.gltf")
    json.dump(doc, open(bare, "w"))
    hs = []
    for p in (path, bare):
        h = C.c_void_p()
        err = C.create_string_buffer(256)
        assert hip_lib.spcbpt_gltf_load(p.encode(), C.byref(h), err, 256) == 0, err.value
        hs.append(h)
    assert _desc_bytes(hip_lib, hs[0], pkg) == _desc_bytes(hip_lib, hs[1], pkg)
    mp, mn = C.POINTER(pkg.api.MeshLight)(), C.c_int()
    assert hip_lib.spcbpt_scene_file_mesh_lights(hs[1], C.byref(mp), C.byref(mn)) == 0 and mn.value == 0
    assert hip_lib.spcbpt_scene_file_mesh_lights(hs[0], C.byref(mp), C.byref(mn)) == 0 and mn.value == 2
    for h in hs:
        hip_lib.spcbpt_scene_file_free(h)


def test_gltf_emissive_texture_and_double_sided_warn_and_patches_fit(hip_lib, pkg, tmp_path):
    sc = _two_lamp_scene(pkg)
    sc.lights[0]["div_level"] = 14                      # 196 of the 200 patch subspaces: two left for each mesh light
    path = pkg.scenes.write_gltf(sc, str(tmp_path), "warn")
    doc = json.load(open(path))
    doc["materials"][3]["emissiveTexture"] = {"index": 0}
    doc["materials"][4]["doubleSided"] = True
    doc["materials"].append({"name": "unused", "emissiveFactor": [1, 1, 1]})     # used by no triangle: not a light
    json.dump(doc, open(path, "w"))
    back, warn = pkg.load_gltf(path, emissive=True)
    assert "emissiveTexture is not honoured" in warn and "doubleSided is not honoured" in warn and "mat3" in warn and "mat4" in warn
    assert [m["material"] for m in back.mesh_lights] == [3, 4]
    assert [m["n_patches"] for m in back.mesh_lights] == [2, 2] and "patch subspaces each" in warn


def _areas64(V, F):
    V = np.asarray(V, np.float32).astype(np.float64)
    e1, e2 = V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]
    return 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)


@pytest.mark.parametrize("subdiv,n_patches", [(2, 4), (3, 16), (0, 7)])
def test_table_of_a_sphere_against_float64(hip_lib, pkg, subdiv, n_patches):
    V, F = pkg.scenes.icosphere((0.3, -0.2, 1.0), 0.7, subdiv)
    rng = np.random.default_rng(5)
    F = F[rng.permutation(len(F))]                      # the table's order must not depend on the caller's
    t = pkg.api.mesh_light_table(V, F, n_patches)
    n = len(F)
    a = _areas64(V, F)
    assert len(t["tri"]) == n and sorted(t["tri"]) == list(range(n)) and t["n_patches"] == n_patches
    assert abs(t["area"] - a.sum()) <= 1e-6 * a.sum()      # (the library takes the edges as the device holds them: float32 differences, 2^-24 each)
    cmf = t["cmf"].astype(np.float64)
    assert (np.diff(cmf) >= 0).all() and t["cmf"][-1] == np.float32(1.0) and cmf[0] > 0
    share = np.diff(np.concatenate([[0.0], cmf]))
    assert np.abs(share - a[t["tri"]] / a.sum()).max() <= 1e-6
    assert np.abs(t["tri_area"] - a[t["tri"]]).max() <= 1e-6 * a.max()
    # patches: non-decreasing along the table, every one in use, areas within a factor two of equal
    assert (np.diff(t["patch"]) >= 0).all() and (np.diff(t["patch"]) <= 1).all()
    assert sorted(set(t["patch"])) == list(range(n_patches))
    pa = np.array([a[t["tri"]][t["patch"] == k].sum() for k in range(n_patches)])
    assert pa.max() <= 2.0 * a.sum() / n_patches and pa.min() >= 0.5 * a.sum() / n_patches, pa / (a.sum() / n_patches)
    # a patch is a run of the Morton curve: its triangles lie together (mean distance to the patch centroid well under the sphere's)
    if subdiv >= 2:
        c = np.asarray(V)[F].mean(1)
        spread = np.mean([np.linalg.norm(c[t["tri"]][t["patch"] == k] - c[t["tri"]][t["patch"] == k].mean(0), axis=1).mean() for k in range(n_patches)])
        assert spread < 0.75 * np.linalg.norm(c - c.mean(0), axis=1).mean()


def test_table_drops_degenerate_triangles_and_fills_every_patch(hip_lib, pkg):
    V = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (2, 0, 0), (5, 5, 5), (5, 5, 6), (5, 6, 5)], np.float32)
    F = np.array([(0, 1, 2), (0, 1, 3), (4, 5, 6), (1, 1, 2), (4, 6, 5)], np.uint32)   # 1: collinear, 3: a repeated corner
    t = pkg.api.mesh_light_table(V, F, 8)
    assert sorted(t["tri"]) == [0, 2, 4] and t["n_patches"] == 3 and sorted(t["patch"]) == [0, 1, 2]
    assert t["cmf"][-1] == 1.0 and abs(t["area"] - 1.5) < 1e-12
    # one huge and many small triangles: no patch stays empty although the big one overshoots several cuts
    V2, F2 = pkg.scenes.icosphere((0, 0, 0), 0.01, 1)
    V2 = np.concatenate([V2, [(10, 0, 0), (20, 0, 0), (10, 10, 0)]])
    F2 = np.concatenate([F2, [(len(V2) - 3, len(V2) - 2, len(V2) - 1)]]).astype(np.uint32)
    t2 = pkg.api.mesh_light_table(V2, F2, 5)
    assert sorted(set(t2["patch"])) == [0, 1, 2, 3, 4]
    # nothing with area: an empty table, not an error code
    assert len(pkg.api.mesh_light_table(V, F[[1, 3]], 4)["tri"]) == 0
    assert hip_lib.spcbpt_mesh_light_table(None, 3, None, 1, 1, None, None, None, None, None, None) == -1


def test_scene_helpers(pkg):
    q = pkg.scenes.cornell_box(div_level=1)
    m = pkg.scenes.quad_lights_as_mesh(q)
    assert m.lights == [] and len(m.mesh_lights) == 1 and m.indices.shape[0] == q.indices.shape[0] + 2
    lamp = pkg.scenes.lamp_floor()
    F = lamp.indices[lamp.tri_material == 1]
    a = _areas64(lamp.vertices, F)
    assert len(a) == 4 and a.max() / a.min() > 1.3
    # closed and outward: the face normals' area-weighted sum vanishes, and every face looks away from the centroid
    V = lamp.vertices.astype(np.float64)
    n = np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]])
    assert np.abs(n.sum(0)).max() < 1e-6
    assert (np.einsum("ij,ij->i", n, V[F].mean(1) - V[np.unique(F)].mean(0)) > 0).all()
    sph = pkg.scenes.cornell_sphere_lamp()
    assert (sph.tri_material == 3).sum() == 320 and sph.lights == []
