"""ctypes binding of include/spcbpt.h — the C ABI of the MI355X SPCBPT hot path.

The host-side mirror of the reference's driver (optixPathTracer.cpp:491-635):
``Renderer.launch("light trace" | "SPCBPT_eye" | "pt" | "pretrace")`` keeps the
four names `sutil::Scene::switchRaygen` dispatches on (sutil/Scene.cpp:1642-1789).
Nothing here falls back to a CPU path: if libspcbpt_hip.so is missing or no HIP
device is present the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

NUM_SUBSPACE = 1000
NUM_SUBSPACE_LIGHTSOURCE = 200
CONNECTION_N = 3
# spcbpt_set_environment_mode flags (include/spcbpt.h)
ENV_EYE_SEES_SKY = 1
ENV_PT_SKY_SHADOW_ALONG_DIR = 2
# spcbpt_debug_unit: the form word of CONNECT / EYE_STEP / SKY_MISS (include/spcbpt.h: SPCBPT_UNIT_FORM_*) and where it and the eye
# vertex's own light-tree label `lsub` sit in the input record, per op; the output words the forms add
UNIT_FORM_REFERENCE, UNIT_FORM_CACHED, UNIT_FORM_CACHED_PLAIN = 0, 1, 2
UNIT_FORMS = dict(reference=UNIT_FORM_REFERENCE, cached=UNIT_FORM_CACHED, cached_plain=UNIT_FORM_CACHED_PLAIN)
UNIT_FORM_WORD = {6: 49, 7: 34, 8: 32}     # CONNECT (in 52), EYE_STEP (in 36), SKY_MISS (in 34: two words behind today's 32); lsub follows
UNIT_CONNECT_NULL_WORD = 4                  # CONNECT with out_words >= 5: 1 where null_connection(_direction) calls the pair null
UNIT_EYE_STEP_LSUB_WORD = 39                # EYE_STEP out: the new vertex's own light-tree label (cached forms)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libspcbpt_hip.so")
# the opt-in approximate-arithmetic build of the same sources (csrc/Makefile: libspcbpt_hip_fast.so; spcbpt_build_arithmetic() == "approx").
# A process picks it with SPCBPT_LIB=<this path> before the first load_library(); never the default.
FAST_LIB_PATH = os.path.join(_HERE, "csrc", "libspcbpt_hip_fast.so")


class Material(C.Structure):
    _fields_ = [("base_color", C.c_float * 3), ("metallic", C.c_float), ("roughness", C.c_float),
                ("specular", C.c_float), ("specular_tint", C.c_float), ("subsurface", C.c_float),
                ("sheen", C.c_float), ("sheen_tint", C.c_float), ("clearcoat", C.c_float),
                ("clearcoat_gloss", C.c_float), ("albedo_tex", C.c_int32), ("brdf", C.c_int32)]


class Texture(C.Structure):
    _fields_ = [("rgba", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32)]


class QuadLight(C.Structure):
    _fields_ = [("position", C.c_float * 3), ("u", C.c_float * 3), ("v", C.c_float * 3),
                ("emission", C.c_float * 3), ("div_level", C.c_int32)]


class MeshLight(C.Structure):   # spcbpt_mesh_light
    _fields_ = [("material", C.c_int32), ("emission", C.c_float * 3), ("n_patches", C.c_int32)]


class DenoiseParams(C.Structure):   # spcbpt_denoise_params
    _fields_ = [("iterations", C.c_int32), ("sigma_c", C.c_float), ("sigma_n", C.c_float), ("sigma_x", C.c_float)]


class GuideParams(C.Structure):   # spcbpt_guide_params
    _fields_ = [("max_bounces", C.c_int32), ("roughness_max", C.c_float), ("metallic_min", C.c_float)]


GUIDE_MAX_BOUNCES, GUIDE_ROUGHNESS_MAX, GUIDE_METALLIC_MIN = 4, 0.1, 0.9   # SPCBPT_GUIDE_*: dials, not tuned against any image
DENOISE_GUIDES = {"first_hit": 0, "reflected": 1}                          # SPCBPT_GUIDES_*


class ReprojectParams(C.Structure):   # spcbpt_reproject_params
    _fields_ = [("sigma_n", C.c_float), ("sigma_x", C.c_float), ("max_history", C.c_float)]


class DisplayParams(C.Structure):   # spcbpt_display_params
    _fields_ = [("op", C.c_int32), ("flags", C.c_uint32), ("ev", C.c_float), ("key", C.c_float), ("low_fraction", C.c_float),
                ("high_fraction", C.c_float), ("ev_bias", C.c_float), ("ev_min", C.c_float), ("ev_max", C.c_float), ("adapt", C.c_float),
                ("white", C.c_float)]


# spcbpt_display: tone operators, flag bits and sources (include/spcbpt.h)
TONE_OPS = {"film": 0, "reinhard": 1, "aces": 2, "linear": 3}
DISPLAY_AUTO = 1
DISPLAY_HISTOGRAM = 2
DISPLAY_SOURCES = {"film": 0, "denoised": 1, "robust": 2, "history": 3, "bloom": 4, "local": 5}   # "bloom": spcbpt_display and spcbpt_local_tone only (the plane of Renderer.bloom); "local": spcbpt_display only (the plane of Renderer.local_tone)
DISPLAY_COUNTERS = 258


class BloomParams(C.Structure):   # spcbpt_bloom_params
    _fields_ = [("levels", C.c_int32), ("strength", C.c_float), ("spread", C.c_float), ("threshold", C.c_float), ("clamp", C.c_float)]


class LocalToneParams(C.Structure):   # spcbpt_local_tone_params
    _fields_ = [("cell", C.c_int32), ("range", C.c_float), ("blur", C.c_int32), ("compress", C.c_float), ("detail", C.c_float), ("anchor", C.c_float)]


class FilmErrorStats(C.Structure):   # spcbpt_film_error_stats
    _fields_ = [("pixels", C.c_int64), ("mean", C.c_double), ("max", C.c_double)]

    def as_dict(self):
        return {"pixels": int(self.pixels), "mean": float(self.mean), "max": float(self.max)}


class AdaptiveParams(C.Structure):   # spcbpt_adaptive_params
    _fields_ = [("target_error", C.c_float), ("min_samples", C.c_uint32), ("max_samples", C.c_uint32)]


class SceneDesc(C.Structure):
    _fields_ = [("vertices", C.c_void_p), ("texcoords", C.c_void_p), ("n_vertices", C.c_int32),
                ("indices", C.c_void_p), ("tri_material", C.c_void_p), ("n_triangles", C.c_int32),
                ("materials", C.POINTER(Material)), ("n_materials", C.c_int32),
                ("textures", C.POINTER(Texture)), ("n_textures", C.c_int32),
                ("lights", C.POINTER(QuadLight)), ("n_lights", C.c_int32)]


class TreeNode(C.Structure):
    _fields_ = [("mid", C.c_float * 3), ("child", C.c_int32 * 8), ("label", C.c_int32),
                ("type", C.c_int32), ("leaf", C.c_int32)]


class LightTraceParams(C.Structure):
    _fields_ = [("num_core", C.c_int32), ("core_padding", C.c_int32), ("m_per_core", C.c_int32),
                ("core_begin", C.c_int32), ("core_count", C.c_int32), ("decorrelate_bsdf_stream", C.c_int32)]


class Counters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "closest_rays", "shadow_rays", "node_visits", "tri_tests", "surface_vertices", "textured_hits",
        "tree_nodes", "cmf_probes", "connections", "gamma_q_reads", "lvc_stores", "pixel_samples",
        "eye_paths", "light_paths")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


# numpy views of the POD records
LIGHT_VERTEX_DTYPE = np.dtype([
    ("position", "<f4", 3), ("pdf", "<f4"), ("normal", "<f4", 3), ("single_pdf", "<f4"),
    ("flux", "<f4", 3), ("rmis_pointer", "<f4"), ("color", "<f4", 3), ("last_lum", "<f4"),
    ("last_position", "<f4", 3), ("last_normal_projection", "<f4"),
    ("material_id", "<i2"), ("subspace_id", "<i2"), ("depth", "<i2"), ("last_zone_id", "<i2"),
    ("path_id", "<u4"), ("pad", "<u4")])
assert LIGHT_VERTEX_DTYPE.itemsize == 96
SUBSPACE_DTYPE = np.dtype([("jump_bias", "<i4"), ("id", "<i4"), ("size", "<i4"), ("sum_pmf", "<f4"), ("q", "<f4")])
TREE_NODE_DTYPE = np.dtype([("mid", "<f4", 3), ("child", "<i4", 8), ("label", "<i4"), ("type", "<i4"), ("leaf", "<i4")])
assert TREE_NODE_DTYPE.itemsize == C.sizeof(TreeNode)

PRETRACE_PATH_DTYPE = np.dtype([("contri", "<f4", 3), ("sample_pdf", "<f4"), ("fix_pdf", "<f4"), ("begin_ind", "<i4"),
                                ("end_ind", "<i4"), ("choice_id", "<i4"), ("pixel_id", "<i4", 2), ("valid", "<i4"), ("pad", "<i4")])
PRETRACE_NODE_DTYPE = np.dtype([("a_position", "<f4", 3), ("b_position", "<f4", 3), ("a_dir", "<f4", 3), ("b_dir", "<f4", 3),
                                ("a_normal", "<f4", 3), ("b_normal", "<f4", 3), ("peak_pdf", "<f4"), ("path_id", "<i4"),
                                ("label_a", "<i4"), ("label_b", "<i4"), ("valid", "<i4"), ("light_source", "<i4")])
assert PRETRACE_PATH_DTYPE.itemsize == 48 and PRETRACE_NODE_DTYPE.itemsize == 96

# Algorithmic byte constants of SURVEY.md 8(d) (fixed by the survey, not tuned).
BYTES = dict(node=64, tri=48, hit=72, mat=144, tex=16, tree=56, cmf=4, sub=20, jump=4, lvc=120, gq=4, lvcw=121, fb=36)


# The same events at the record sizes THIS build fetches (csrc/layout.h): 64-B quantised 4-wide node, 48-B triangle test (+ the
# fourth quad for the hit), 64-B material, 16-B classifier node, 16-B subspace record, 96-B light vertex (32 B of it for the
# shadow ray alone), 16-B radiance store + the film merge (16 R + 16 W + 4 W).  Reported next to the contract number, which
# credits the kernel with bytes it no longer needs.
BYTES_ACTUAL = dict(node=64, tri=48, hit=64, mat=64, tex=16, tree=16, cmf=4, sub=16, jump=4, lvc=96, gq=4, lvcw=96, fb=52)


def source_hash() -> str:
    """csrc/source_hash.py: the hash the Makefile embeds in the library (spcbpt_build_source_hash)."""
    import runpy
    return runpy.run_path(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "source_hash.py"))["source_hash"]()


def kernel_hash() -> str:
    """csrc/source_hash.py: hash of the eye megakernel's device sources (what profiles/traffic_latest.json is valid for)."""
    import runpy
    return runpy.run_path(os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "source_hash.py"))["kernel_hash"]()


def algorithmic_bytes(c: dict, table: Optional[dict] = None) -> int:
    """bytes = sum_e count_e * B_e  (SURVEY.md 8(d))."""
    b = table or BYTES
    return (c["node_visits"] * b["node"] + c["tri_tests"] * b["tri"] + c["surface_vertices"] * (b["hit"] + b["mat"])
            + c["textured_hits"] * b["tex"] + c["tree_nodes"] * b["tree"] + c["cmf_probes"] * b["cmf"]
            + c["connections"] * (b["sub"] + b["jump"] + b["lvc"] + 2 * b["mat"]) + c["gamma_q_reads"] * b["gq"]
            + c["lvc_stores"] * b["lvcw"] + c["pixel_samples"] * b["fb"])


@dataclass
class Scene:
    """Flat triangle soup + materials + quad lights, as the C ABI takes it."""
    vertices: np.ndarray            # (nv, 3) f32
    indices: np.ndarray             # (nt, 3) u32
    tri_material: np.ndarray        # (nt,) i32
    materials: List[dict]
    lights: List[dict]
    texcoords: Optional[np.ndarray] = None   # (nv, 2) f32
    textures: List[np.ndarray] = field(default_factory=list)  # (h, w, 4) u8
    camera: dict = field(default_factory=dict)  # eye, lookat, up, fov
    name: str = "scene"
    environment: Optional[dict] = None   # rgba (h, w, 4) f32 as a .hdr stores it (row 0 = top), center (3,), radius: Renderer.set_environment(**scene.environment)
    # emissive meshes as area lights (spcbpt_create_lit): dicts material (index into `materials`), emission (3,), n_patches (default 4)
    mesh_lights: List[dict] = field(default_factory=list)

    def mesh_light_array(self):
        """The ctypes array spcbpt_create_lit takes (at least one element, so that the pointer is never NULL)."""
        ml = (MeshLight * max(1, len(self.mesh_lights)))()
        for k, d in enumerate(self.mesh_lights):
            ml[k].material = int(d["material"])
            ml[k].emission[:] = [float(x) for x in d["emission"]]
            ml[k].n_patches = int(d.get("n_patches", 4))
        return ml

    def desc(self):
        """Returns (SceneDesc, keepalive)."""
        v = np.ascontiguousarray(self.vertices, dtype=np.float32)
        i = np.ascontiguousarray(self.indices, dtype=np.uint32)
        m = np.ascontiguousarray(self.tri_material, dtype=np.int32)
        assert v.ndim == 2 and v.shape[1] == 3 and i.ndim == 2 and i.shape[1] == 3 and m.shape[0] == i.shape[0]
        assert int(i.max(initial=0)) < v.shape[0] and int(m.max(initial=0)) < len(self.materials)
        t = None if self.texcoords is None else np.ascontiguousarray(self.texcoords, dtype=np.float32)
        mats = (Material * max(1, len(self.materials)))()
        for k, d in enumerate(self.materials):
            mm = mats[k]
            mm.base_color[:] = [float(x) for x in d.get("color", (1, 1, 1))]
            mm.metallic = d.get("metallic", 0.0)
            mm.roughness = d.get("roughness", 0.5)
            # q17: the .scene hand-off keeps MaterialData() defaults for the other Disney parameters
            mm.specular = d.get("specular", 0.5)
            mm.specular_tint = d.get("specular_tint", 0.0)
            mm.subsurface = d.get("subsurface", 0.0)
            mm.sheen = d.get("sheen", 0.0)
            mm.sheen_tint = d.get("sheen_tint", 0.5)
            mm.clearcoat = d.get("clearcoat", 0.0)
            mm.clearcoat_gloss = d.get("clearcoat_gloss", 1.0)
            mm.albedo_tex = d.get("albedo_tex", 0)
            mm.brdf = int(d.get("brdf", 0))   # Pbr::brdf (MaterialData.h:99): `brdf <int>` of a .scene material block
            assert 0 <= mm.albedo_tex <= len(self.textures)
        texs = (Texture * max(1, len(self.textures)))()
        tex_keep = []
        for k, im in enumerate(self.textures):
            im = np.ascontiguousarray(im, dtype=np.uint8)
            assert im.ndim == 3 and im.shape[2] == 4
            tex_keep.append(im)
            texs[k].rgba = im.ctypes.data
            texs[k].height, texs[k].width = im.shape[0], im.shape[1]
        ls = (QuadLight * max(1, len(self.lights)))()
        for k, d in enumerate(self.lights):
            ls[k].position[:] = [float(x) for x in d["position"]]
            ls[k].u[:] = [float(x) for x in d["u"]]
            ls[k].v[:] = [float(x) for x in d["v"]]
            ls[k].emission[:] = [float(x) for x in d["emission"]]
            ls[k].div_level = int(d.get("div_level", 1))
        assert sum(int(d.get("div_level", 1)) ** 2 for d in self.lights) <= NUM_SUBSPACE_LIGHTSOURCE
        sd = SceneDesc()
        sd.vertices = v.ctypes.data
        sd.texcoords = None if t is None else t.ctypes.data
        sd.n_vertices = v.shape[0]
        sd.indices = i.ctypes.data
        sd.tri_material = m.ctypes.data
        sd.n_triangles = i.shape[0]
        sd.materials = mats
        sd.n_materials = len(self.materials)
        sd.textures = texs
        sd.n_textures = len(self.textures)
        sd.lights = ls
        sd.n_lights = len(self.lights)
        return sd, (v, i, m, t, mats, texs, tex_keep, ls)


def load_scene_file(scene_path: str, data_root: str):
    """Parses a reference-format `.scene` file with the library's C++ loader (spcbpt_scene_file_load) and copies the
    result into a Scene.  Returns (scene, warnings)."""
    lib = load_library()
    h = C.c_void_p()
    rc = lib.spcbpt_scene_file_load(scene_path.encode(), data_root.encode(), C.byref(h))
    if rc != 0:
        raise SpcbptError(f"spcbpt_scene_file_load({scene_path}) failed ({rc})")
    return _scene_from_handle(lib, h, os.path.basename(scene_path))


def load_gltf(path: str, lights=None, emissive=False):
    """Reads a glTF 2.0 file (.gltf / .glb) with the library's C++ reader (spcbpt_gltf_load).  `lights` (list of quad-light
    dicts) replaces whatever the file's `extras.spcbpt_quad_lights` holds.  emissive=True: the file's emissive materials become
    the scene's mesh lights (spcbpt_scene_file_mesh_lights); by default they are ignored, as before.  Returns (scene, warnings)."""
    lib = load_library()
    h = C.c_void_p()
    err = C.create_string_buffer(512)
    rc = lib.spcbpt_gltf_load(path.encode(), C.byref(h), err, 512)
    if rc != 0:
        raise SpcbptError(f"spcbpt_gltf_load({path}) failed ({rc}): {err.value.decode()}")
    scene, warn = _scene_from_handle(lib, h, os.path.basename(path), mesh_lights=emissive)
    if lights is not None:
        scene.lights = list(lights)
    return scene, warn


def _scene_from_handle(lib, h, name, mesh_lights=False):
    try:
        d = SceneDesc()
        lib.spcbpt_scene_file_desc(h, C.byref(d))
        nv, nt = d.n_vertices, d.n_triangles
        as_np = lambda ptr, ct, n: np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ct)), shape=(n,)).copy() if n else np.zeros(0, ct)
        V = as_np(d.vertices, C.c_float, 3 * nv).reshape(-1, 3)
        UV = as_np(d.texcoords, C.c_float, 2 * nv).reshape(-1, 2)
        I = as_np(d.indices, C.c_uint32, 3 * nt).reshape(-1, 3)
        M = as_np(d.tri_material, C.c_int32, nt)
        mats = []
        for k in range(d.n_materials):
            m = d.materials[k]
            mats.append(dict(color=tuple(m.base_color), metallic=m.metallic, roughness=m.roughness, albedo_tex=m.albedo_tex, brdf=m.brdf))
        lights = []
        for k in range(d.n_lights):
            l = d.lights[k]
            lights.append(dict(position=tuple(l.position), u=tuple(l.u), v=tuple(l.v), emission=tuple(l.emission), div_level=l.div_level))
        texs = []
        for k in range(d.n_textures):
            t = d.textures[k]
            texs.append(np.ctypeslib.as_array(C.cast(t.rgba, C.POINTER(C.c_uint8)), shape=(t.height, t.width, 4)).copy())
        eye, look, up = (np.zeros(3, np.float32) for _ in range(3))
        fov, w, hh = C.c_float(), C.c_int(), C.c_int()
        lib.spcbpt_scene_file_camera(h, _fp(eye), _fp(look), _fp(up), C.byref(fov), C.byref(w), C.byref(hh))
        cam = dict(eye=tuple(eye), lookat=tuple(look), up=tuple(up), fov=fov.value, width=w.value, height=hh.value)
        env = None
        ep, ew, eh, er = C.c_void_p(), C.c_int(), C.c_int(), C.c_float()
        ec = np.zeros(3, np.float32)
        if hasattr(lib, "spcbpt_scene_file_environment"):    # (absent only from an older SPCBPT_LIB build)
            lib.spcbpt_scene_file_environment(h, C.byref(ep), C.byref(ew), C.byref(eh), _fp(ec), C.byref(er))
        if ew.value > 0:
            px = np.ctypeslib.as_array(C.cast(ep, C.POINTER(C.c_float)), shape=(eh.value, ew.value, 4)).copy()
            env = dict(rgba=px, center=ec.copy(), radius=float(er.value))
        warn = lib.spcbpt_scene_file_warnings(h).decode()
        mls = []
        if mesh_lights:
            mp, mn = C.POINTER(MeshLight)(), C.c_int()
            lib.spcbpt_scene_file_mesh_lights(h, C.byref(mp), C.byref(mn))
            mls = [dict(material=int(mp[k].material), emission=tuple(mp[k].emission), n_patches=int(mp[k].n_patches)) for k in range(mn.value)]
        return Scene(vertices=V, indices=I, tri_material=M, materials=mats, lights=lights, texcoords=UV, textures=texs,
                     camera=cam, name=name, environment=env, mesh_lights=mls), warn
    finally:
        lib.spcbpt_scene_file_free(h)


def mesh_light_table(vertices, triangles, n_patches):
    """The sampling table spcbpt_create_lit builds for one mesh light (spcbpt_mesh_light_table; needs no GPU): `triangles` = (n, 3)
    vertex indices of the light's triangles.  Returns dict tri (table order -> row of `triangles`), cmf, patch, tri_area, area, n_patches."""
    lib = load_library()
    v = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
    i = np.ascontiguousarray(triangles, dtype=np.uint32).reshape(-1, 3)
    n = i.shape[0]
    tri, cmf, patch, ta = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float32)
    area, npch = C.c_double(), C.c_int32()
    k = lib.spcbpt_mesh_light_table(v.ctypes.data, v.shape[0], i.ctypes.data, n, int(n_patches), tri.ctypes.data, cmf.ctypes.data,
                                    patch.ctypes.data, ta.ctypes.data, C.byref(area), C.byref(npch))
    if k < 0:
        raise SpcbptError(f"spcbpt_mesh_light_table failed ({k})")
    return dict(tri=tri[:k].copy(), cmf=cmf[:k].copy(), patch=patch[:k].copy(), tri_area=ta[:k].copy(), area=area.value, n_patches=npch.value)


def camera_frame(eye, lookat, up, fov_y_deg, aspect):
    """sutil::Camera::UVWFrame (sutil/Camera.cpp:34-45) in float32."""
    f = np.float32
    eye, lookat, up = (np.asarray(a, dtype=f) for a in (eye, lookat, up))
    W = lookat - eye
    wlen = np.sqrt(np.dot(W, W), dtype=f)
    U = np.cross(W, up).astype(f)
    U = U * (f(1.0) / np.sqrt(np.dot(U, U), dtype=f))
    V = np.cross(U, W).astype(f)
    V = V * (f(1.0) / np.sqrt(np.dot(V, V), dtype=f))
    vlen = wlen * f(np.tan(f(0.5) * f(fov_y_deg) * f(np.pi) / f(180.0)))
    V = V * vlen
    U = U * (vlen * f(aspect))
    return U.astype(f), V.astype(f), W.astype(f)


def camera_splat(eye, U, V, W, width, height, point):
    """spcbpt_camera_splat: where `point` lands on a width x height film seen through (eye, U, V, W), and the importance the
    light-tracing estimator "lt" gives it.  Returns (dx, dy, px, py, weight), or None when the point does not project inside
    the image.  Host code in float32 -- the function the splat kernel calls; no GPU needed."""
    lib = load_library()
    a = [np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (eye, U, V, W, point)]
    dx, dy, we = C.c_float(0.0), C.c_float(0.0), C.c_float(0.0)
    px, py = C.c_int(-1), C.c_int(-1)
    if not lib.spcbpt_camera_splat(_fp(a[0]), _fp(a[1]), _fp(a[2]), _fp(a[3]), int(width), int(height), _fp(a[4]),
                                   C.byref(dx), C.byref(dy), C.byref(px), C.byref(py), C.byref(we)):
        return None
    return dx.value, dy.value, px.value, py.value, we.value


def camera_lens_ray_host(eye, U, V, W, width, height, xy, jitter, lens, radius, focus):
    """spcbpt_camera_lens_ray_host: the thin-lens camera's eye side for n samples -- pixels xy (n, 2) int, jitter (n, 2) and lens
    numbers (n, 2) in [0, 1) -> (origin (n, 3), direction (n, 3)) float32.  Host code in float32 -- the function the lens kernels
    call; no GPU needed.  radius 0 gives `eye` and the pinhole direction."""
    lib = load_library()
    a = [np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (eye, U, V, W)]
    xy = np.ascontiguousarray(xy, dtype=np.int32).reshape(-1, 2)
    n = xy.shape[0]
    jitter = np.ascontiguousarray(jitter, dtype=np.float32).reshape(n, 2)
    lens = np.ascontiguousarray(lens, dtype=np.float32).reshape(n, 2)
    origin, direction = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    rc = lib.spcbpt_camera_lens_ray_host(_fp(a[0]), _fp(a[1]), _fp(a[2]), _fp(a[3]), int(width), int(height), n, xy.ctypes.data_as(C.POINTER(C.c_int32)),
                                         _fp(jitter), _fp(lens), float(radius), float(focus), _fp(origin), _fp(direction))
    if rc != 0:
        raise ValueError(f"spcbpt_camera_lens_ray_host: bad argument (rc={rc})")
    return origin, direction


def camera_splat_lens(eye, U, V, W, width, height, points, lens, radius, focus):
    """spcbpt_camera_splat_lens: the thin-lens camera's light side for n world points (n, 3), each seen through the lens point of its
    lens numbers (n, 2).  Returns (inside (n,) bool, dxdy (n, 2), pixel (n, 2) int32, weight (n,)); rows with inside False hold zeros
    and pixel -1.  Host code in float32 -- the function the "lt" kernels call; no GPU needed.  radius 0 is camera_splat."""
    lib = load_library()
    a = [np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (eye, U, V, W)]
    points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    n = points.shape[0]
    lens = np.ascontiguousarray(lens, dtype=np.float32).reshape(n, 2)
    dxdy, pixel = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.int32)
    weight, inside = np.zeros(n, np.float32), np.zeros(n, np.int32)
    rc = lib.spcbpt_camera_splat_lens(_fp(a[0]), _fp(a[1]), _fp(a[2]), _fp(a[3]), int(width), int(height), n, _fp(points), _fp(lens), float(radius), float(focus),
                                      _fp(dxdy), pixel.ctypes.data_as(C.POINTER(C.c_int32)), _fp(weight), inside.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise ValueError(f"spcbpt_camera_splat_lens: bad argument (rc={rc})")
    return inside.astype(bool), dxdy, pixel, weight


def lens_sample_host(index, subframe, with_jitter=True):
    """spcbpt_lens_sample_host: (jx, jy, u1, u2) as a lens kernel draws them -- for pixel index y * width + x (with_jitter: the jitter
    is 0.5 and draws nothing at subframe 0) or for cache slot `index` of "lt" (with_jitter=False).  `index` may be an array: (n, 4)."""
    lib = load_library()
    idx = np.atleast_1d(np.asarray(index, dtype=np.uint32))
    out = np.zeros((idx.size, 4), np.float32)
    row = (C.c_float * 4)()
    for i, v in enumerate(idx.ravel()):
        lib.spcbpt_lens_sample_host(int(v), int(subframe), 1 if with_jitter else 0, row)
        out[i] = row[:]
    return out if np.ndim(index) else out[0]


def denoise_host(accum, albedo, normal_depth, eye, U, V, W, iterations=5, sigma_c=0.0, sigma_n=0.0, sigma_x=0.0):
    """spcbpt_denoise_host: the a-trous denoiser of Renderer.denoise on (h, w, 4) float32 arrays as read_accum / read_features give
    them, seen through the camera (eye, U, V, W).  Host code in float32 -- the per-pixel function the kernels run; no GPU needed.
    A sigma <= 0 takes its default.  Returns the denoised (h, w, 4) image; the inputs are not written."""
    lib = load_library()
    a = [np.ascontiguousarray(v, dtype=np.float32) for v in (accum, albedo, normal_depth)]
    h, w = a[0].shape[:2]
    if any(v.shape != (h, w, 4) for v in a):
        raise SpcbptError("denoise_host: accum, albedo and normal_depth must be (h, w, 4) arrays of one size")
    cam = [np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (eye, U, V, W)]
    out = np.zeros((h, w, 4), dtype=np.float32)
    p = DenoiseParams(int(iterations), float(sigma_c), float(sigma_n), float(sigma_x))
    rc = lib.spcbpt_denoise_host(_fp(a[0]), _fp(a[1]), _fp(a[2]), *[_fp(v) for v in cam], w, h, C.byref(p), _fp(out))
    if rc != 0:
        raise SpcbptError(f"denoise_host failed ({rc})")
    return out


def guide_step_host(dir, normal, material, specular_tint, test_normal, roughness_max=GUIDE_ROUGHNESS_MAX, metallic_min=GUIDE_METALLIC_MIN):
    """spcbpt_guide_step_host: the per-bounce arithmetic of Renderer.launch_guides over n records -- dir, normal and test_normal (n, 3),
    material (n, 6): base r, g, b, metallic, roughness, specular; specular_tint (n,).  Returns (followed (n,) bool, reflected (n, 3), tint
    (n, 3), unfolded (n, 3)): the roughness / metallic rule, R = dir - 2 (N.dir) N, the mirror's Fresnel colour, and test_normal carried
    back through the mirror.  Host code in float32 -- the functions the kernel runs; no GPU needed."""
    lib = load_library()
    d, N, m, st, tn = (np.ascontiguousarray(x, dtype=np.float32) for x in (dir, normal, material, specular_tint, test_normal))
    n = len(st)
    if n < 1 or d.shape != (n, 3) or N.shape != (n, 3) or tn.shape != (n, 3) or m.shape != (n, 6) or st.shape != (n,):
        raise SpcbptError("guide_step_host: dir, normal and test_normal must be (n, 3), material (n, 6), specular_tint (n,)")
    p = GuideParams(0, float(roughness_max), float(metallic_min))
    followed = np.zeros(n, np.int32)
    R, tint, unf = (np.zeros((n, 3), np.float32) for _ in range(3))
    rc = lib.spcbpt_guide_step_host(n, _fp(d), _fp(N), _fp(m), _fp(st), _fp(tn), C.byref(p), followed.ctypes.data_as(C.POINTER(C.c_int32)), _fp(R), _fp(tint), _fp(unf))
    if rc != 0:
        raise SpcbptError(f"guide_step_host failed ({rc})")
    return followed != 0, R, tint, unf


def denoise_variance_host(accum, m2n, albedo, normal_depth, eye, U, V, W, iterations=5, sigma_v=0.0, sigma_n=0.0, sigma_x=0.0):
    """spcbpt_denoise_variance_host: the variance-guided a-trous denoiser of Renderer.denoise_variance on (h, w, 4) float32 arrays as
    read_accum / read_film_moments / read_features give them.  Host code in float32 -- the per-pixel function the kernels run; no GPU
    needed.  A sigma <= 0 takes its default.  Returns the denoised (h, w, 4) image; the inputs are not written."""
    lib = load_library()
    a = [np.ascontiguousarray(v, dtype=np.float32) for v in (accum, m2n, albedo, normal_depth)]
    h, w = a[0].shape[:2]
    if any(v.shape != (h, w, 4) for v in a):
        raise SpcbptError("denoise_variance_host: accum, m2n, albedo and normal_depth must be (h, w, 4) arrays of one size")
    cam = [np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (eye, U, V, W)]
    out = np.zeros((h, w, 4), dtype=np.float32)
    p = DenoiseParams(int(iterations), float(sigma_v), float(sigma_n), float(sigma_x))
    rc = lib.spcbpt_denoise_variance_host(_fp(a[0]), _fp(a[1]), _fp(a[2]), _fp(a[3]), *[_fp(v) for v in cam], w, h, C.byref(p), _fp(out))
    if rc != 0:
        raise SpcbptError(f"denoise_variance_host failed ({rc})")
    return out


def history_reproject_host(camera, normal_depth, history_camera, history_normal_depth, history_rgbn, sigma_n=0.0, sigma_x=0.0, max_history=0.0, diag=0.0):
    """spcbpt_history_reproject_host: the prior of Renderer.history_reproject on (h, w, 4) float32 arrays -- the current view's
    normal / depth plane, the history's, and the history image (rgb, n) -- with the two cameras as (eye, U, V, W).  Host code in float32
    -- the per-pixel function the kernel runs; no GPU needed.  A parameter <= 0 takes its default (sigma_x: a fraction of `diag`).
    Returns the (h, w, 4) prior (rgb, m); the inputs are not written."""
    lib = load_library()
    a = [np.ascontiguousarray(v, dtype=np.float32) for v in (normal_depth, history_normal_depth, history_rgbn)]
    h, w = a[0].shape[:2]
    if any(v.shape != (h, w, 4) for v in a):
        raise SpcbptError("history_reproject_host: the three planes must be (h, w, 4) arrays of one size")
    cam = [np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in tuple(camera) + tuple(history_camera)]
    if len(cam) != 8:
        raise SpcbptError("history_reproject_host: a camera is (eye, U, V, W)")
    out = np.zeros((h, w, 4), dtype=np.float32)
    p = ReprojectParams(float(sigma_n), float(sigma_x), float(max_history))
    rc = lib.spcbpt_history_reproject_host(*[_fp(v) for v in cam[:4]], _fp(a[0]), *[_fp(v) for v in cam[4:]], _fp(a[1]), _fp(a[2]), w, h,
                                           C.byref(p), C.c_float(diag), _fp(out))
    if rc != 0:
        raise SpcbptError(f"history_reproject_host failed ({rc})")
    return out


def history_resolve_host(prior, accum, frames):
    """spcbpt_history_resolve_host: the blend of Renderer.history_resolve on (..., 4) float32 arrays -- the prior (or None: no prior)
    and the film's mean of `frames` frames.  The per-pixel function the kernel runs; no GPU needed.  Returns (rgb, m + frames)."""
    lib = load_library()
    a = np.ascontiguousarray(accum, dtype=np.float32)
    r = None if prior is None else np.ascontiguousarray(prior, dtype=np.float32)
    if a.shape[-1] != 4 or (r is not None and r.shape != a.shape):
        raise SpcbptError("history_resolve_host: prior and accum must be (..., 4) arrays of one shape")
    if int(frames) < 0 or int(frames) >= 2**32:
        raise SpcbptError("history_resolve_host: frames out of range")
    out = np.zeros(a.shape, dtype=np.float32)
    rc = lib.spcbpt_history_resolve_host(_fp(r) if r is not None else None, _fp(a), int(frames), a.size // 4, _fp(out))
    if rc != 0:
        raise SpcbptError(f"history_resolve_host failed ({rc})")
    return out


def history_reproject_var_host(camera, normal_depth, history_camera, history_normal_depth, history_rgbn, history_var, sigma_n=0.0, sigma_x=0.0, max_history=0.0, diag=0.0):
    """spcbpt_history_reproject_var_host: history_reproject_host with the history's variance plane `history_var` ((h, w, 4): the
    per-channel variance of history_rgbn's rgb) as a second payload of the same taps.  Returns (prior, prior_var): the (h, w, 4) prior
    (rgb, m), bit for bit history_reproject_host's, and its variance (V_r, V_g, V_b, 0).  No GPU needed; the inputs are not written."""
    lib = load_library()
    a = [np.ascontiguousarray(v, dtype=np.float32) for v in (normal_depth, history_normal_depth, history_rgbn, history_var)]
    h, w = a[0].shape[:2]
    if any(v.shape != (h, w, 4) for v in a):
        raise SpcbptError("history_reproject_var_host: the four planes must be (h, w, 4) arrays of one size")
    cam = [np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in tuple(camera) + tuple(history_camera)]
    if len(cam) != 8:
        raise SpcbptError("history_reproject_var_host: a camera is (eye, U, V, W)")
    out, out_var = np.zeros((h, w, 4), dtype=np.float32), np.zeros((h, w, 4), dtype=np.float32)
    p = ReprojectParams(float(sigma_n), float(sigma_x), float(max_history))
    rc = lib.spcbpt_history_reproject_var_host(*[_fp(v) for v in cam[:4]], _fp(a[0]), *[_fp(v) for v in cam[4:]], _fp(a[1]), _fp(a[2]), _fp(a[3]), w, h,
                                               C.byref(p), C.c_float(diag), _fp(out), _fp(out_var))
    if rc != 0:
        raise SpcbptError(f"history_reproject_var_host failed ({rc})")
    return out, out_var


def history_resolve_var_host(prior, prior_var, accum, m2n, frames):
    """spcbpt_history_resolve_var_host: history_resolve_host with the variance of the blend -- the prior and its variance (both None: no
    prior), the film's mean of `frames` frames and its moments plane as read_film_moments gives it.  Returns (resolved, resolved_var):
    (rgb, m + frames) and (V_r, V_g, V_b, 0).  No GPU needed."""
    lib = load_library()
    a, m = (np.ascontiguousarray(v, dtype=np.float32) for v in (accum, m2n))
    r = None if prior is None else np.ascontiguousarray(prior, dtype=np.float32)
    rv = None if prior_var is None else np.ascontiguousarray(prior_var, dtype=np.float32)
    if a.shape[-1] != 4 or m.shape != a.shape or any(v is not None and v.shape != a.shape for v in (r, rv)):
        raise SpcbptError("history_resolve_var_host: the planes must be (..., 4) arrays of one shape")
    if int(frames) < 0 or int(frames) >= 2**32:
        raise SpcbptError("history_resolve_var_host: frames out of range")
    out, out_var = np.zeros(a.shape, dtype=np.float32), np.zeros(a.shape, dtype=np.float32)
    rc = lib.spcbpt_history_resolve_var_host(_fp(r) if r is not None else None, _fp(rv) if rv is not None else None, _fp(a), _fp(m), int(frames), a.size // 4,
                                             _fp(out), _fp(out_var))
    if rc != 0:
        raise SpcbptError(f"history_resolve_var_host failed ({rc})")
    return out, out_var


def history_denoise_host(resolved, resolved_var, albedo, normal_depth, eye, U, V, W, iterations=5, sigma_v=0.0, sigma_n=0.0, sigma_x=0.0):
    """spcbpt_history_denoise_host: the variance-guided a-trous denoiser of Renderer.history_denoise on (h, w, 4) float32 arrays as
    read_history / read_history_variance / read_features give them.  Host code in float32 -- the per-pixel function the kernels run; no
    GPU needed.  A sigma <= 0 takes its default.  Returns the denoised (h, w, 4) image; the inputs are not written."""
    lib = load_library()
    a = [np.ascontiguousarray(v, dtype=np.float32) for v in (resolved, resolved_var, albedo, normal_depth)]
    h, w = a[0].shape[:2]
    if any(v.shape != (h, w, 4) for v in a):
        raise SpcbptError("history_denoise_host: resolved, resolved_var, albedo and normal_depth must be (h, w, 4) arrays of one size")
    cam = [np.ascontiguousarray(v, dtype=np.float32).reshape(3) for v in (eye, U, V, W)]
    out = np.zeros((h, w, 4), dtype=np.float32)
    p = DenoiseParams(int(iterations), float(sigma_v), float(sigma_n), float(sigma_x))
    rc = lib.spcbpt_history_denoise_host(_fp(a[0]), _fp(a[1]), _fp(a[2]), _fp(a[3]), *[_fp(v) for v in cam], w, h, C.byref(p), _fp(out))
    if rc != 0:
        raise SpcbptError(f"history_denoise_host failed ({rc})")
    return out


SPLAT_ATOMIC, SPLAT_ORDERED = 0, 1   # spcbpt_set_splat_order


def splat_sum_host(rgb, pixel, width, height):
    """spcbpt_splat_sum_host: the ordered splat sum of "lt" on the host -- (height, width, 3) float32, every pixel +0.0 plus the rgb of
    its records in ascending record index, one float32 addition each; records with a pixel index < 0 or >= width * height are skipped."""
    lib = load_library()
    c = np.ascontiguousarray(rgb, np.float32).reshape(-1, 3)
    p = np.ascontiguousarray(pixel, np.int32).reshape(-1)
    if len(c) != len(p):
        raise SpcbptError("splat_sum_host: rgb must hold three floats per entry of pixel")
    out = np.empty((int(height), int(width), 3), np.float32)
    rc = lib.spcbpt_splat_sum_host(_fp(c) if len(p) else None, p.ctypes.data_as(C.POINTER(C.c_int32)) if len(p) else None, len(p), int(width), int(height), _fp(out))
    if rc != 0:
        raise SpcbptError(f"splat_sum_host failed ({rc})")
    return out


def film_moments_update_host(mean_before, sample, subframe, m2n):
    """spcbpt_film_moments_update_host: one merge's update of the moment plane `m2n` ((..., 4) float32, C-contiguous, updated IN PLACE)
    from the film before the merge and the frame's samples (same shape).  The per-pixel function the kernel runs; no GPU needed."""
    lib = load_library()
    a, x = (np.ascontiguousarray(v, dtype=np.float32) for v in (mean_before, sample))
    if not (isinstance(m2n, np.ndarray) and m2n.dtype == np.float32 and m2n.flags["C_CONTIGUOUS"]):
        raise SpcbptError("film_moments_update_host: m2n must be a C-contiguous float32 array (it is updated in place)")
    if a.shape != m2n.shape or x.shape != m2n.shape or m2n.shape[-1] != 4:
        raise SpcbptError("film_moments_update_host: mean_before, sample and m2n must be (..., 4) arrays of one shape")
    rc = lib.spcbpt_film_moments_update_host(_fp(a), _fp(x), int(subframe), m2n.size // 4, _fp(m2n))
    if rc != 0:
        raise SpcbptError(f"film_moments_update_host failed ({rc})")
    return m2n


def film_buckets_update_host(sample, subframe, planes):
    """spcbpt_film_buckets_update_host: one merge's update of the bucket planes `planes` ((K, ..., 4) float32, C-contiguous, updated IN
    PLACE; K = 3 .. 32) from the frame's samples ((..., 4)): bucket subframe % K takes the sample, subframe 0 restarts all K.  The
    per-pixel function the kernel runs; no GPU needed."""
    lib = load_library()
    x = np.ascontiguousarray(sample, dtype=np.float32)
    if not (isinstance(planes, np.ndarray) and planes.dtype == np.float32 and planes.flags["C_CONTIGUOUS"]):
        raise SpcbptError("film_buckets_update_host: planes must be a C-contiguous float32 array (it is updated in place)")
    if planes.ndim < 2 or planes.shape[1:] != x.shape or x.shape[-1] != 4:
        raise SpcbptError("film_buckets_update_host: sample must be (..., 4) and planes (K, ..., 4)")
    rc = lib.spcbpt_film_buckets_update_host(_fp(x), int(subframe), planes.shape[0], x.size // 4, _fp(planes))
    if rc != 0:
        raise SpcbptError(f"film_buckets_update_host failed ({rc})")
    return planes


def film_merge_batch_host(samples, subframes, accum, m2n=None, planes=None):
    """spcbpt_film_merge_batch_host: the batched merge of launch_eye_batch_film on the host.  `samples` is (n, ..., 4) float32, the
    frames' samples in batch order, `subframes` their n subframe indices; `accum` ((..., 4)), `m2n` ((..., 4), None = no moments) and
    `planes` ((K, ..., 4), None = no buckets) are C-contiguous float32 arrays updated IN PLACE.  The per-pixel function the kernel
    runs; no GPU needed."""
    lib = load_library()
    x = np.ascontiguousarray(samples, dtype=np.float32)
    sf = np.ascontiguousarray(subframes, dtype=np.uint32).reshape(-1)
    for name, a in (("accum", accum), ("m2n", m2n), ("planes", planes)):
        if a is not None and not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]):
            raise SpcbptError(f"film_merge_batch_host: {name} must be a C-contiguous float32 array (it is updated in place)")
    if x.ndim < 2 or x.shape[-1] != 4 or x.shape[0] != len(sf) or accum.shape != x.shape[1:]:
        raise SpcbptError("film_merge_batch_host: samples must be (n, ..., 4) with n = len(subframes) and accum (..., 4)")
    if m2n is not None and m2n.shape != accum.shape:
        raise SpcbptError("film_merge_batch_host: m2n must have accum's shape")
    if planes is not None and (planes.ndim < 2 or planes.shape[1:] != accum.shape):
        raise SpcbptError("film_merge_batch_host: planes must be (K, ..., 4) over accum's shape")
    rc = lib.spcbpt_film_merge_batch_host(_fp(x), sf.ctypes.data_as(C.POINTER(C.c_uint32)), len(sf), accum.size // 4,
                                          planes.shape[0] if planes is not None else 0, _fp(accum),
                                          _fp(m2n) if m2n is not None else None, _fp(planes) if planes is not None else None)
    if rc != 0:
        raise SpcbptError(f"film_merge_batch_host failed ({rc})")
    return accum


def robust_resolve_host(planes, strength=1.0):
    """spcbpt_robust_resolve_host: the median-of-means resolve of bucket planes ((K, ..., 4) float32 as read_film_buckets gives them) at
    `strength` in [0, 8].  Returns (..., 4) float32: (r, g, b, w) with w the number of buckets kept.  The per-pixel function the
    kernel runs; no GPU needed."""
    lib = load_library()
    p = np.ascontiguousarray(planes, dtype=np.float32)
    if p.ndim < 2 or p.shape[-1] != 4:
        raise SpcbptError("robust_resolve_host: planes must be (K, ..., 4)")
    out = np.zeros(p.shape[1:], np.float32)
    rc = lib.spcbpt_robust_resolve_host(_fp(p), p.shape[0], out.size // 4, float(strength), _fp(out))
    if rc != 0:
        raise SpcbptError(f"robust_resolve_host failed ({rc})")
    return out


def display_params(op="film", ev=None, auto=False, histogram=False, **fields):
    """A spcbpt_display_params: the library's defaults (spcbpt_display_default_params), then `op` (a name of TONE_OPS or its number), the
    flag bits from `auto` / `histogram`, a manual `ev` and any further field by name (key, low_fraction, high_fraction, ev_bias, ev_min,
    ev_max, adapt, white, flags)."""
    lib = load_library()
    p = DisplayParams()
    if lib.spcbpt_display_default_params(C.byref(p)) != 0:
        raise SpcbptError("display_default_params failed")
    p.op = TONE_OPS[op] if isinstance(op, str) else int(op)
    p.flags = (DISPLAY_AUTO if auto else 0) | (DISPLAY_HISTOGRAM if histogram else 0)
    if ev is not None:
        p.ev = float(ev)
    names = {n for n, _ in DisplayParams._fields_}
    for k, v in fields.items():
        if k not in names:
            raise SpcbptError(f"display_params: no field '{k}'")
        setattr(p, k, v)
    return p


def display_host(img, have_prev=False, prev_ev=0.0, **params):
    """spcbpt_display_host: the display transform of an (..., 4) float32 image on the host, parameters as display_params takes them.
    Returns (rgba8 (..., 4) uint8, histogram (258,) uint32, ev).  The per-pixel code the kernels run; no GPU needed."""
    lib = load_library()
    x = np.ascontiguousarray(img, dtype=np.float32)
    if x.ndim < 1 or x.shape[-1] != 4:
        raise SpcbptError("display_host: the image must be (..., 4)")
    p = display_params(**params)
    out = np.zeros(x.shape, np.uint8)
    hist = np.zeros(DISPLAY_COUNTERS, np.uint32)
    ev = C.c_float()
    rc = lib.spcbpt_display_host(_fp(x), x.size // 4, C.byref(p), int(bool(have_prev)), float(prev_ev), out.ctypes.data, hist.ctypes.data, C.byref(ev))
    if rc != 0:
        raise SpcbptError(f"display_host failed ({rc})")
    return out, hist, float(ev.value)


def bloom_params(**fields):
    """A spcbpt_bloom_params: the library's defaults (spcbpt_bloom_default_params), then any field by name (levels, strength, spread,
    threshold, clamp)."""
    lib = load_library()
    p = BloomParams()
    if lib.spcbpt_bloom_default_params(C.byref(p)) != 0:
        raise SpcbptError("bloom_default_params failed")
    names = {n for n, _ in BloomParams._fields_}
    for k, v in fields.items():
        if k not in names:
            raise SpcbptError(f"bloom_params: no field '{k}'")
        setattr(p, k, v)
    return p


def bloom_host(img, **params):
    """spcbpt_bloom_host: the bloom stage of an (h, w, 4) float32 image on the host, parameters as bloom_params takes them.  Returns the
    (h, w, 4) float32 result.  The per-texel code the kernels run; no GPU needed."""
    lib = load_library()
    x = np.ascontiguousarray(img, dtype=np.float32)
    if x.ndim != 3 or x.shape[-1] != 4:
        raise SpcbptError("bloom_host: the image must be (h, w, 4)")
    p = bloom_params(**params)
    out = np.zeros(x.shape, np.float32)
    rc = lib.spcbpt_bloom_host(_fp(x), x.shape[1], x.shape[0], C.byref(p), _fp(out))
    if rc != 0:
        raise SpcbptError(f"bloom_host failed ({rc})")
    return out


def local_tone_params(**fields):
    """A spcbpt_local_tone_params: the library's defaults (spcbpt_local_tone_default_params), then any field by name (cell, range, blur,
    compress, detail, anchor)."""
    lib = load_library()
    p = LocalToneParams()
    if lib.spcbpt_local_tone_default_params(C.byref(p)) != 0:
        raise SpcbptError("local_tone_default_params failed")
    names = {n for n, _ in LocalToneParams._fields_}
    for k, v in fields.items():
        if k not in names:
            raise SpcbptError(f"local_tone_params: no field '{k}'")
        setattr(p, k, v)
    return p


def local_tone_host(img, **params):
    """spcbpt_local_tone_host: the local tone stage of an (h, w, 4) float32 image on the host, parameters as local_tone_params takes
    them.  Returns the (h, w, 4) float32 result.  The per-pixel and per-node code the kernels run; no GPU needed."""
    lib = load_library()
    x = np.ascontiguousarray(img, dtype=np.float32)
    if x.ndim != 3 or x.shape[-1] != 4:
        raise SpcbptError("local_tone_host: the image must be (h, w, 4)")
    p = local_tone_params(**params)
    out = np.zeros(x.shape, np.float32)
    rc = lib.spcbpt_local_tone_host(_fp(x), x.shape[1], x.shape[0], C.byref(p), _fp(out))
    if rc != 0:
        raise SpcbptError(f"local_tone_host failed ({rc})")
    return out


def local_tone_math_host(values, which):
    """spcbpt_local_tone_math_host (for the tests): lt_log2 (which = 0) or lt_exp2 (which = 1) of the stage over a float32 array."""
    lib = load_library()
    x = np.ascontiguousarray(values, dtype=np.float32)
    out = np.zeros(x.shape, np.float32)
    rc = lib.spcbpt_local_tone_math_host(_fp(x), x.size, int(which), _fp(out))
    if rc != 0:
        raise SpcbptError(f"local_tone_math_host failed ({rc})")
    return out


def film_error_host(accum, m2n):
    """spcbpt_film_error_host: {"pixels", "mean", "max"} of the relative standard error over the pixels with n >= 2, from (..., 4)
    float32 arrays as read_accum / read_film_moments give them.  The per-pixel function the kernel runs; no GPU needed."""
    lib = load_library()
    a, m = (np.ascontiguousarray(v, dtype=np.float32) for v in (accum, m2n))
    if a.shape != m.shape or a.shape[-1] != 4:
        raise SpcbptError("film_error_host: accum and m2n must be (..., 4) arrays of one shape")
    out = FilmErrorStats()
    rc = lib.spcbpt_film_error_host(_fp(a), _fp(m), a.size // 4, C.byref(out))
    if rc != 0:
        raise SpcbptError(f"film_error_host failed ({rc})")
    return out.as_dict()


def adaptive_select_host(accum, m2n, tile_samples, target_error, min_samples=0, max_samples=0):
    """spcbpt_adaptive_select_host: the tile errors and the tile list of adaptive sampling from (h, w, 4) float32 arrays as read_accum /
    read_film_moments give them and the per-tile sample counts ((tiles_y, tiles_x) or flat; tiles are 8x8 pixels, x-major).  Returns
    {"error": (tiles_y, tiles_x) float32, "tiles": ascending uint32 list}.  The per-tile functions the kernels run; no GPU needed."""
    lib = load_library()
    a, m = (np.ascontiguousarray(v, dtype=np.float32) for v in (accum, m2n))
    if a.shape != m.shape or a.ndim != 3 or a.shape[-1] != 4:
        raise SpcbptError("adaptive_select_host: accum and m2n must be (h, w, 4) arrays of one shape")
    h, w = a.shape[:2]
    ty, tx = (h + 7) // 8, (w + 7) // 8
    n = np.ascontiguousarray(tile_samples, dtype=np.uint32).reshape(-1)
    if n.size != tx * ty:
        raise SpcbptError(f"adaptive_select_host: tile_samples must hold {ty} x {tx} counts")
    err = np.zeros((ty, tx), dtype=np.float32)
    tiles = np.zeros(tx * ty, dtype=np.uint32)
    count = C.c_int(0)
    p = AdaptiveParams(float(target_error), int(min_samples), int(max_samples))
    rc = lib.spcbpt_adaptive_select_host(_fp(a), _fp(m), w, h, n.ctypes.data, C.byref(p), _fp(err), tiles.ctypes.data, C.byref(count))
    if rc != 0:
        raise SpcbptError(f"adaptive_select_host failed ({rc})")
    return {"error": err, "tiles": tiles[:count.value].copy()}


def single_leaf_tree(label=0):
    t = np.zeros(1, dtype=TREE_NODE_DTYPE)
    t[0]["leaf"] = 1
    t[0]["label"] = label
    return t


class SpcbptError(RuntimeError):
    pass


_lib = None


class ViewerState(C.Structure):  # spcbpt_viewer_state
    _fields_ = [("eye", C.c_float * 3), ("lookat", C.c_float * 3), ("up", C.c_float * 3),
                ("U", C.c_float * 3), ("V", C.c_float * 3), ("W", C.c_float * 3),
                ("fov_y", C.c_float), ("aspect", C.c_float), ("width", C.c_int32), ("height", C.c_int32),
                ("subframe_index", C.c_uint32), ("alg_id", C.c_int32), ("should_close", C.c_int32),
                ("one_frame_render_only", C.c_int32), ("camera_changed", C.c_int32), ("render_fps", C.c_float)]


KEY = {"ESCAPE": 256, "SPACE": 32, "C": 67, "G": 71, "P": 80, "W": 87}   # GLFW key codes the reference's keyCallback tests
BUTTON = {"left": 0, "right": 1, "middle": 2}


class Viewer:
    """Mirror of the spcbpt_viewer_* entry points (row f3): the reference application's event handling and render loop
    without a window.  `renderer` may be None (state machine only, no GPU)."""

    def __init__(self, renderer, eye, lookat, up, fov_y, width, height):
        self.lib = load_library()
        self.renderer = renderer
        self.h = C.c_void_p()
        rc = self.lib.spcbpt_viewer_create(renderer.h if renderer is not None else None, _fp(np.asarray(eye, np.float32)),
                                           _fp(np.asarray(lookat, np.float32)), _fp(np.asarray(up, np.float32)),
                                           C.c_float(fov_y), width, height, C.byref(self.h))
        if rc:
            raise SpcbptError(f"viewer_create failed ({rc})")

    def close(self):
        if self.h:
            self.lib.spcbpt_viewer_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc:
            msg = self.lib.spcbpt_last_error(self.renderer.h) if self.renderer is not None else None
            raise SpcbptError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def mouse_button(self, button, action, x, y):
        self._chk(self.lib.spcbpt_viewer_mouse_button(self.h, BUTTON.get(button, button), int(action), float(x), float(y)), "mouse_button")

    def cursor_pos(self, x, y):
        self._chk(self.lib.spcbpt_viewer_cursor_pos(self.h, float(x), float(y)), "cursor_pos")

    def scroll(self, yscroll):
        self._chk(self.lib.spcbpt_viewer_scroll(self.h, 0.0, float(yscroll)), "scroll")

    def window_size(self, w, h):
        self._chk(self.lib.spcbpt_viewer_window_size(self.h, int(w), int(h)), "window_size")

    def iconify(self, on):
        self._chk(self.lib.spcbpt_viewer_iconify(self.h, int(on)), "iconify")

    def key(self, key, action=1):
        self._chk(self.lib.spcbpt_viewer_key(self.h, KEY.get(key, key), int(action)), "key")

    def set_fps(self, fps):
        self._chk(self.lib.spcbpt_viewer_set_fps(self.h, C.c_float(fps)), "set_fps")

    def set_light_ahead(self, on):
        self._chk(self.lib.spcbpt_viewer_set_light_ahead(self.h, int(on)), "viewer_set_light_ahead")

    def set_reproject(self, on):
        """spcbpt_viewer_set_reproject: carry the shown image across camera moves (off by default); flipping it restarts the accumulation."""
        self._chk(self.lib.spcbpt_viewer_set_reproject(self.h, int(bool(on))), "viewer_set_reproject")

    def get_reproject(self):
        """{"on", "live"}: the switch, and whether a prior is live (the resolved image differs from the film)."""
        on, live = C.c_int32(), C.c_int32()
        self._chk(self.lib.spcbpt_viewer_get_reproject(self.h, C.byref(on), C.byref(live)), "viewer_get_reproject")
        return {"on": int(on.value), "live": int(live.value)}

    def set_denoise(self, on):
        """spcbpt_viewer_set_denoise: follow every shown frame's resolve with history_denoise (defaults); display read_denoised().  Needs
        set_reproject(True); switches the context's film moments on (and back); flipping it restarts the accumulation."""
        self._chk(self.lib.spcbpt_viewer_set_denoise(self.h, int(bool(on))), "viewer_set_denoise")

    def get_denoise(self) -> bool:
        on = C.c_int32()
        self._chk(self.lib.spcbpt_viewer_get_denoise(self.h, C.byref(on)), "viewer_get_denoise")
        return bool(on.value)

    def set_pipeline(self, mode: int):
        """0 the reference's order, 1 next light pass beside the eye kernel, 2 (default) next frame traced while this one is shown."""
        self._chk(self.lib.spcbpt_viewer_set_pipeline(self.h, int(mode)), "viewer_set_pipeline")

    def frame(self):
        self._chk(self.lib.spcbpt_viewer_frame(self.h), "viewer_frame")

    def state(self):
        s = ViewerState()
        self._chk(self.lib.spcbpt_viewer_get_state(self.h, C.byref(s)), "get_state")
        d = {k: (np.array(getattr(s, k), dtype=np.float32) if k in ("eye", "lookat", "up", "U", "V", "W") else getattr(s, k))
             for k, _ in ViewerState._fields_}
        d["alg"] = self.lib.spcbpt_viewer_alg_name(s.alg_id).decode()
        return d

    def replay(self, events):
        """events as in oracle/ref_viewer.cpp: rows (type, a, b, c) with 0 press(button, x, y), 1 release(button),
        2 cursor(x, y), 3 scroll(yscroll), 4 key W at render_fps a.  Returns the camera (eye, lookat, up, U, V, W) after each."""
        out = np.zeros((len(events), 18), np.float32)
        for i, (t, a, b, c) in enumerate(np.asarray(events, np.float64)):
            t = int(t)
            if t == 0: self.mouse_button(int(a), 1, b, c)
            elif t == 1: self.mouse_button(int(a), 0, b, c)
            elif t == 2: self.cursor_pos(b, c)
            elif t == 3: self.scroll(a)
            elif t == 4:
                self.set_fps(a)
                self.key("W", 1)
            s = self.state()
            out[i] = np.concatenate([s["eye"], s["lookat"], s["up"], s["U"], s["V"], s["W"]])
        return out


def hdr_load(path: str):
    """(h, w, 4) float32 raster of a Radiance .hdr file, decoded as the reference's HDRLoader (scene_shift.cpp:334-500); row 0 = top."""
    lib = load_library()
    w, h = C.c_int(), C.c_int()
    rc = lib.spcbpt_hdr_load(os.fsencode(path), C.byref(w), C.byref(h), None, 0)
    if rc:
        raise SpcbptError(f"hdr_load({path}) failed ({rc})")
    px = np.zeros((h.value, w.value, 4), np.float32)
    rc = lib.spcbpt_hdr_load(os.fsencode(path), C.byref(w), C.byref(h), px.ctypes.data, px.size)
    if rc:
        raise SpcbptError(f"hdr_load({path}) failed ({rc})")
    return px


def image_load(path: str):
    """RGBA8 image (h, w, 4) of a JPEG / PNG / binary PPM file, decoded as the reference's stbi_load(..., STBI_rgb_alpha)."""
    lib = load_library()
    w, h = C.c_int(), C.c_int()
    rc = lib.spcbpt_image_load(os.fsencode(path), C.byref(w), C.byref(h), None, 0)
    if rc:
        raise SpcbptError(f"image_load({path}) failed ({rc})")
    px = np.zeros((h.value, w.value, 4), np.uint8)
    rc = lib.spcbpt_image_load(os.fsencode(path), C.byref(w), C.byref(h), px.ctypes.data, px.nbytes)
    if rc:
        raise SpcbptError(f"image_load({path}) failed ({rc})")
    return px


def checkpoint_write(directory: str, eye_tree, light_tree, q, gamma):
    """Context-free writer of the reference's checkpoint files (spcbpt_checkpoint_write)."""
    lib = load_library()
    et = np.ascontiguousarray(eye_tree, dtype=TREE_NODE_DTYPE)
    lt = np.ascontiguousarray(light_tree, dtype=TREE_NODE_DTYPE)
    q = np.ascontiguousarray(q, dtype=np.float32)
    g = np.ascontiguousarray(gamma, dtype=np.float32)
    assert q.size == NUM_SUBSPACE and g.size == NUM_SUBSPACE * NUM_SUBSPACE
    rc = lib.spcbpt_checkpoint_write(os.fsencode(directory), et.ctypes.data, et.shape[0], lt.ctypes.data, lt.shape[0], q.ctypes.data, g.ctypes.data)
    if rc:
        raise SpcbptError(f"checkpoint_write failed ({rc})")


def checkpoint_read(directory: str, current_gamma=None, cap=1 << 20):
    """Context-free reader (tree_load + load_Q_file + load_Gamma_file): returns (eye_tree, light_tree, Q, Gamma).  With
    `current_gamma` the emitter-subspace columns keep its values, as load_Gamma_file does."""
    lib = load_library()
    et = np.zeros(cap, dtype=TREE_NODE_DTYPE)
    lt = np.zeros(cap, dtype=TREE_NODE_DTYPE)
    q = np.zeros(NUM_SUBSPACE, dtype=np.float32)
    g = np.zeros(NUM_SUBSPACE * NUM_SUBSPACE, dtype=np.float32) if current_gamma is None else \
        np.ascontiguousarray(current_gamma, dtype=np.float32).reshape(-1).copy()
    ne, nl = C.c_int(), C.c_int()
    rc = lib.spcbpt_checkpoint_read(os.fsencode(directory), et.ctypes.data, C.byref(ne), cap, lt.ctypes.data, C.byref(nl), cap,
                                    q.ctypes.data, g.ctypes.data, 0 if current_gamma is None else 1)
    if rc:
        raise SpcbptError(f"checkpoint_read failed ({rc})")
    return et[:ne.value].copy(), lt[:nl.value].copy(), q, g.reshape(NUM_SUBSPACE, NUM_SUBSPACE)


def gamma_to_cmf(gamma):
    lib = load_library()
    g = np.ascontiguousarray(gamma, dtype=np.float32).reshape(-1)
    out = np.zeros_like(g)
    lib.spcbpt_gamma_to_cmf(g.ctypes.data, out.ctypes.data)
    return out.reshape(NUM_SUBSPACE, NUM_SUBSPACE)


def load_library(path: str = LIB_PATH):
    """Loads libspcbpt_hip.so.  Raises if it has not been built — there is no CPU fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if os.environ.get("SPCBPT_LIB"):   # developer A/B runs: another build of the same ABI (no source-hash check)
        path = os.environ["SPCBPT_LIB"]
    if not os.path.exists(path):
        raise SpcbptError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's).
    # Importing torch first makes this library bind to the runtime torch uses, so torch.distributed (RCCL) buffers
    # and the context's buffers live in the same HIP context.  Without torch the system runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)   # libspcbpt_mgpu.so resolves the C ABI against this handle
    # a library built from other sources than the tree holds must not be tested or benchmarked silently
    try:
        lib.spcbpt_build_source_hash.restype = C.c_char_p
        built = lib.spcbpt_build_source_hash().decode()
    except AttributeError:
        built = "none"
    if path in (LIB_PATH, FAST_LIB_PATH) and built != source_hash() and not os.environ.get("SPCBPT_ALLOW_STALE_LIB"):
        raise SpcbptError(f"{path} was built from other sources (library {built}, tree {source_hash()}): run `make -C spcbpt-optix7_amd/csrc`")
    vp, i32, u32, f32p = C.c_void_p, C.c_int, C.c_uint32, C.POINTER(C.c_float)
    sig = {
        "spcbpt_create": [C.POINTER(SceneDesc), i32, C.POINTER(vp)],
        "spcbpt_create_lit": [C.POINTER(SceneDesc), C.POINTER(MeshLight), i32, i32, C.POINTER(vp)],
        "spcbpt_mesh_light_struct_size": [],
        "spcbpt_light_info": [vp, i32, C.POINTER(i32), C.POINTER(C.c_float), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)],
        "spcbpt_mesh_light_table": [vp, i32, vp, i32, i32, vp, vp, vp, vp, C.POINTER(C.c_double), C.POINTER(i32)],
        "spcbpt_scene_file_mesh_lights": [vp, C.POINTER(C.POINTER(MeshLight)), C.POINTER(i32)],
        "spcbpt_destroy": [vp],
        "spcbpt_set_camera": [vp, f32p, f32p, f32p, f32p],
        "spcbpt_set_camera_lookat": [vp, f32p, f32p, f32p, C.c_float, C.c_float],
        "spcbpt_resize": [vp, i32, i32],
        "spcbpt_set_subspace": [vp, vp, i32, vp, i32, vp, vp],
        "spcbpt_set_light_trace": [vp, C.POINTER(LightTraceParams)],
        "spcbpt_launch": [vp, C.c_char_p, u32, i32, i32, i32],
        "spcbpt_build_sampler": [vp],
        "spcbpt_build_sampler_batch": [vp, C.c_int],
        "spcbpt_launch_eye_batch": [vp, i32, C.POINTER(u32), i32, i32, i32],
        "spcbpt_launch_light_batch": [vp, u32, i32],
        "spcbpt_lvc_export": [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(i32)],
        "spcbpt_lvc_import": [vp, vp, i32, i32],
        "spcbpt_set_environment": [vp, vp, i32, i32, vp, C.c_float],
        "spcbpt_get_environment": [vp, C.POINTER(i32), C.POINTER(i32), f32p, C.POINTER(C.c_float), C.POINTER(i32)],
        "spcbpt_set_environment_mode": [vp, i32],
        "spcbpt_get_environment_mode": [vp, C.POINTER(i32)],
        "spcbpt_hdr_load": [C.c_char_p, C.POINTER(i32), C.POINTER(i32), vp, C.c_size_t],
        "spcbpt_lvc_set_capacity": [vp, i32],
        "spcbpt_lvc_get_capacity": [vp, C.POINTER(i32), C.POINTER(i32)],
        "spcbpt_lvc_read": [vp, vp, i32, C.POINTER(i32)],
        "spcbpt_sampler_read": [vp, vp, vp, vp, i32, C.POINTER(i32), C.POINTER(i32)],
        "spcbpt_read_accum": [vp, vp],
        "spcbpt_read_frame": [vp, vp],
        "spcbpt_accum_device_ptr": [vp, C.POINTER(vp)],
        "spcbpt_clear_accum": [vp],
        "spcbpt_get_counters": [vp, C.POINTER(Counters)],
        "spcbpt_reset_counters": [vp],
        "spcbpt_debug_phase_clocks": [vp, C.POINTER(C.c_uint64)],
        "spcbpt_set_connection_sampler": [vp, i32],
        "spcbpt_debug_unit": [vp, i32, vp, i32, vp, i32, i32, vp, i32],
        "spcbpt_debug_trace_bench": [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp],
        "spcbpt_debug_trace_pool": [vp, i32, vp, vp, vp, vp, vp, vp, vp],
        "spcbpt_debug_spill_arm": [vp],
        "spcbpt_debug_spill_count": [vp, C.POINTER(C.c_uint64), C.POINTER(i32)],
        "spcbpt_enable_counters": [vp, i32],
        "spcbpt_stream": [vp, C.POINTER(vp)],
        "spcbpt_sync": [vp], "spcbpt_sync_film": [vp], "spcbpt_merge_deferred": [vp, i32], "spcbpt_launch_deferred": [vp, C.c_char_p, u32, i32, i32, i32],
        "spcbpt_sync_light": [vp],
        "spcbpt_set_light_ahead": [vp, i32],
        "spcbpt_get_pipeline_state": [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)],
        "spcbpt_reuse_sampler": [vp],
        "spcbpt_read_film": [vp, vp, vp],
        "spcbpt_debug_batch_scratch": [vp, C.POINTER(C.c_int64), C.POINTER(i32), C.POINTER(i32)],
        "spcbpt_debug_read_sampling_tables": [vp, vp, i32, vp, vp],
        "spcbpt_lvc_import_wait": [vp],
        "spcbpt_kernel_time": [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(i32)],
        "spcbpt_reset_kernel_time": [vp],
        "spcbpt_enable_kernel_timing": [vp, i32],
        "spcbpt_trace_closest": [vp, vp, i32, vp, vp, vp],
        "spcbpt_trace_any": [vp, vp, i32, vp],
        "spcbpt_camera_splat": [f32p, f32p, f32p, f32p, i32, i32, f32p, f32p, f32p, C.POINTER(i32), C.POINTER(i32), f32p],
        "spcbpt_set_lens": [vp, C.c_float, C.c_float],
        "spcbpt_get_lens": [vp, f32p, f32p],
        "spcbpt_camera_lens_ray_host": [f32p, f32p, f32p, f32p, i32, i32, i32, C.POINTER(C.c_int32), f32p, f32p, C.c_float, C.c_float, f32p, f32p],
        "spcbpt_camera_splat_lens": [f32p, f32p, f32p, f32p, i32, i32, i32, f32p, f32p, C.c_float, C.c_float, f32p, C.POINTER(C.c_int32), f32p, C.POINTER(C.c_int32)],
        "spcbpt_lens_sample_host": [C.c_uint32, C.c_uint32, i32, f32p],
        "spcbpt_debug_lens_rays": [vp, C.c_uint32, f32p],
        "spcbpt_set_splat_order": [vp, i32],
        "spcbpt_get_splat_order": [vp, C.POINTER(i32)],
        "spcbpt_read_splat_records": [vp, f32p, C.POINTER(C.c_int32), i32, C.POINTER(i32)],
        "spcbpt_splat_sum_host": [f32p, C.POINTER(C.c_int32), C.c_int64, i32, i32, f32p],
        "spcbpt_launch_features": [vp, u32, i32, i32, i32],
        "spcbpt_read_features": [vp, vp, vp],
        "spcbpt_launch_guides": [vp, u32, i32, i32, i32, C.POINTER(GuideParams)],
        "spcbpt_read_guides": [vp, vp, vp],
        "spcbpt_set_denoise_guides": [vp, i32],
        "spcbpt_guide_params_struct_size": [],
        "spcbpt_guide_step_host": [C.c_int64, f32p, f32p, f32p, f32p, f32p, C.POINTER(GuideParams), C.POINTER(C.c_int32), f32p, f32p, f32p],
        "spcbpt_denoise": [vp, C.POINTER(DenoiseParams)],
        "spcbpt_denoise_params_struct_size": [],
        "spcbpt_read_denoised": [vp, vp, vp],
        "spcbpt_denoise_host": [f32p, f32p, f32p, f32p, f32p, f32p, f32p, i32, i32, C.POINTER(DenoiseParams), f32p],
        "spcbpt_set_film_moments": [vp, i32],
        "spcbpt_get_film_moments": [vp, C.POINTER(i32)],
        "spcbpt_read_film_moments": [vp, vp],
        "spcbpt_film_moments_update_host": [f32p, f32p, u32, C.c_int64, f32p],
        "spcbpt_film_error": [vp, C.POINTER(FilmErrorStats)],
        "spcbpt_film_error_struct_size": [],
        "spcbpt_film_error_host": [f32p, f32p, C.c_int64, C.POINTER(FilmErrorStats)],
        "spcbpt_denoise_variance": [vp, C.POINTER(DenoiseParams)],
        "spcbpt_set_film_buckets": [vp, i32],
        "spcbpt_get_film_buckets": [vp, C.POINTER(i32)],
        "spcbpt_read_film_buckets": [vp, vp],
        "spcbpt_film_buckets_update_host": [f32p, u32, i32, C.c_int64, f32p],
        "spcbpt_film_merge_batch_host": [f32p, C.POINTER(u32), i32, C.c_int64, i32, f32p, f32p, f32p],
        "spcbpt_launch_eye_batch_film": [vp, i32, C.POINTER(u32), i32, i32, i32],
        "spcbpt_robust_resolve": [vp, C.c_float],
        "spcbpt_read_robust": [vp, vp, vp],
        "spcbpt_robust_resolve_host": [f32p, i32, C.c_int64, C.c_float, f32p],
        "spcbpt_display_default_params": [C.POINTER(DisplayParams)],
        "spcbpt_display_params_struct_size": [],
        "spcbpt_display": [vp, i32, C.POINTER(DisplayParams)],
        "spcbpt_display_image": [vp, f32p, i32, i32, C.POINTER(DisplayParams)],
        "spcbpt_read_display": [vp, vp, vp, C.POINTER(C.c_float), C.POINTER(i32), C.POINTER(i32)],
        "spcbpt_display_reset": [vp],
        "spcbpt_display_host": [f32p, C.c_int64, C.POINTER(DisplayParams), i32, C.c_float, vp, vp, C.POINTER(C.c_float)],
        "spcbpt_bloom_default_params": [C.POINTER(BloomParams)],
        "spcbpt_bloom_params_struct_size": [],
        "spcbpt_bloom": [vp, i32, C.POINTER(BloomParams)],
        "spcbpt_bloom_image": [vp, f32p, i32, i32, C.POINTER(BloomParams)],
        "spcbpt_read_bloom": [vp, vp, C.POINTER(i32), C.POINTER(i32)],
        "spcbpt_bloom_host": [f32p, i32, i32, C.POINTER(BloomParams), f32p],
        "spcbpt_local_tone_default_params": [C.POINTER(LocalToneParams)],
        "spcbpt_local_tone_params_struct_size": [],
        "spcbpt_local_tone": [vp, i32, C.POINTER(LocalToneParams)],
        "spcbpt_local_tone_image": [vp, f32p, i32, i32, C.POINTER(LocalToneParams)],
        "spcbpt_read_local_tone": [vp, vp, C.POINTER(i32), C.POINTER(i32)],
        "spcbpt_local_tone_host": [f32p, i32, i32, C.POINTER(LocalToneParams), f32p],
        "spcbpt_local_tone_math_host": [f32p, C.c_int64, i32, f32p],
        "spcbpt_adaptive_params_struct_size": [], "spcbpt_adaptive_begin": [vp, u32], "spcbpt_adaptive_end": [vp],
        "spcbpt_adaptive_select": [vp, C.POINTER(AdaptiveParams), C.POINTER(i32)], "spcbpt_adaptive_set_tiles": [vp, vp, i32],
        "spcbpt_launch_adaptive": [vp, C.c_char_p], "spcbpt_read_adaptive": [vp, vp, vp, vp, i32, C.POINTER(i32)],
        "spcbpt_get_adaptive_state": [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)],
        "spcbpt_adaptive_select_host": [f32p, f32p, i32, i32, vp, C.POINTER(AdaptiveParams), f32p, vp, C.POINTER(i32)],
        "spcbpt_history_capture": [vp, C.c_uint32], "spcbpt_history_reproject": [vp, C.POINTER(ReprojectParams)], "spcbpt_history_resolve": [vp, C.c_uint32],
        "spcbpt_history_reset": [vp], "spcbpt_reproject_params_struct_size": [], "spcbpt_read_history": [vp, vp, vp, vp, vp],
        "spcbpt_history_reproject_host": [f32p, f32p, f32p, f32p, f32p, f32p, f32p, f32p, f32p, f32p, f32p, i32, i32, C.POINTER(ReprojectParams), C.c_float, f32p],
        "spcbpt_history_resolve_host": [f32p, f32p, C.c_uint32, C.c_int64, f32p],
        "spcbpt_history_denoise": [vp, C.POINTER(DenoiseParams)], "spcbpt_read_history_variance": [vp, vp, vp, vp],
        "spcbpt_history_reproject_var_host": [f32p, f32p, f32p, f32p, f32p, f32p, f32p, f32p, f32p, f32p, f32p, f32p, i32, i32, C.POINTER(ReprojectParams), C.c_float, f32p, f32p],
        "spcbpt_history_resolve_var_host": [f32p, f32p, f32p, f32p, C.c_uint32, C.c_int64, f32p, f32p],
        "spcbpt_history_denoise_host": [f32p, f32p, f32p, f32p, f32p, f32p, f32p, f32p, i32, i32, C.POINTER(DenoiseParams), f32p],
        "spcbpt_viewer_set_denoise": [vp, i32], "spcbpt_viewer_get_denoise": [vp, C.POINTER(i32)],
        "spcbpt_viewer_set_reproject": [vp, i32], "spcbpt_viewer_get_reproject": [vp, C.POINTER(i32), C.POINTER(i32)],
        "spcbpt_denoise_variance_host": [f32p, f32p, f32p, f32p, f32p, f32p, f32p, f32p, i32, i32, C.POINTER(DenoiseParams), f32p],
        "spcbpt_preprocess": [vp, i32, i32, i32],
        "spcbpt_set_pretrace": [vp, i32, i32],
        "spcbpt_train_records_count": [vp, C.POINTER(i32), C.POINTER(i32)],
        "spcbpt_train_records_read": [vp, vp, i32, vp, i32],
        "spcbpt_train_records_import": [vp, vp, i32, vp, i32],
        "spcbpt_train_records_clear": [vp],
        "spcbpt_preprocess_stage": [vp, i32, i32],
        "spcbpt_get_gamma": [vp, vp],
        "spcbpt_checkpoint_write": [C.c_char_p, vp, i32, vp, i32, vp, vp],
        "spcbpt_checkpoint_read": [C.c_char_p, vp, C.POINTER(i32), i32, vp, C.POINTER(i32), i32, vp, vp, i32],
        "spcbpt_gamma_to_cmf": [vp, vp],
        "spcbpt_viewer_create": [vp, f32p, f32p, f32p, C.c_float, i32, i32, C.POINTER(vp)],
        "spcbpt_viewer_mouse_button": [vp, i32, i32, C.c_double, C.c_double],
        "spcbpt_viewer_cursor_pos": [vp, C.c_double, C.c_double],
        "spcbpt_viewer_scroll": [vp, C.c_double, C.c_double],
        "spcbpt_viewer_window_size": [vp, i32, i32],
        "spcbpt_viewer_iconify": [vp, i32],
        "spcbpt_viewer_key": [vp, i32, i32],
        "spcbpt_viewer_set_fps": [vp, C.c_float],
        "spcbpt_viewer_set_light_ahead": [vp, i32], "spcbpt_viewer_set_pipeline": [vp, i32],
        "spcbpt_viewer_frame": [vp],
        "spcbpt_viewer_get_state": [vp, C.POINTER(ViewerState)],
        "spcbpt_image_load": [C.c_char_p, C.POINTER(i32), C.POINTER(i32), vp, C.c_size_t],
        "spcbpt_checkpoint_save": [vp, C.c_char_p],
        "spcbpt_checkpoint_load": [vp, C.c_char_p],
        "spcbpt_gltf_load": [C.c_char_p, C.POINTER(vp), C.c_char_p, i32],
        "spcbpt_scene_file_load": [C.c_char_p, C.c_char_p, C.POINTER(vp)],
        "spcbpt_scene_file_desc": [vp, C.POINTER(SceneDesc)],
        "spcbpt_scene_file_camera": [vp, f32p, f32p, f32p, f32p, C.POINTER(i32), C.POINTER(i32)],
        "spcbpt_scene_file_environment": [vp, C.POINTER(vp), C.POINTER(i32), C.POINTER(i32), f32p, C.POINTER(C.c_float)],
        "spcbpt_scene_file_free": [vp],
        "spcbpt_get_subspace": [vp, vp, C.POINTER(i32), i32, vp, C.POINTER(i32), i32, vp, vp],
        "spcbpt_scene_info": [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)],
    }
    for name, args in sig.items():
        if os.environ.get("SPCBPT_LIB") and not hasattr(lib, name):
            continue                   # an older build of the ABI in a developer A/B run
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    lib.spcbpt_viewer_destroy.argtypes = [vp]
    lib.spcbpt_viewer_destroy.restype = None
    lib.spcbpt_viewer_alg_name.argtypes = [i32]
    lib.spcbpt_viewer_alg_name.restype = C.c_char_p
    lib.spcbpt_last_error.argtypes = [vp]
    lib.spcbpt_last_error.restype = C.c_char_p
    lib.spcbpt_build_arithmetic.restype = C.c_char_p
    lib.spcbpt_scene_file_warnings.argtypes = [vp]
    lib.spcbpt_scene_file_warnings.restype = C.c_char_p
    _lib = lib
    return lib


EXPORTED_SYMBOLS = [
    "spcbpt_create", "spcbpt_create_lit", "spcbpt_mesh_light_struct_size", "spcbpt_light_info", "spcbpt_mesh_light_table", "spcbpt_scene_file_mesh_lights", "spcbpt_destroy", "spcbpt_last_error", "spcbpt_set_camera", "spcbpt_set_camera_lookat",
    "spcbpt_resize", "spcbpt_set_subspace", "spcbpt_set_light_trace", "spcbpt_launch", "spcbpt_launch_eye_batch", "spcbpt_launch_eye_batch_film", "spcbpt_film_merge_batch_host", "spcbpt_launch_light_batch", "spcbpt_build_sampler", "spcbpt_build_sampler_batch",
    "spcbpt_lvc_export", "spcbpt_lvc_import", "spcbpt_lvc_set_capacity", "spcbpt_lvc_get_capacity", "spcbpt_set_environment", "spcbpt_get_environment", "spcbpt_set_environment_mode", "spcbpt_get_environment_mode", "spcbpt_hdr_load", "spcbpt_lvc_read", "spcbpt_sampler_read", "spcbpt_read_accum",
    "spcbpt_read_frame", "spcbpt_accum_device_ptr", "spcbpt_clear_accum", "spcbpt_get_counters",
    "spcbpt_reset_counters", "spcbpt_debug_phase_clocks", "spcbpt_debug_spill_arm", "spcbpt_debug_spill_count", "spcbpt_set_connection_sampler", "spcbpt_debug_unit", "spcbpt_debug_trace_bench", "spcbpt_debug_trace_pool",
    "spcbpt_build_source_hash", "spcbpt_build_arithmetic", "spcbpt_abi_struct_sizes", "spcbpt_lvc_export_on", "spcbpt_lvc_import_gathered", "spcbpt_lvc_export_batch_on", "spcbpt_lvc_import_gathered_batch", "spcbpt_film_pack_bands", "spcbpt_film_unpack_bands", "spcbpt_image_size", "spcbpt_get_light_trace", "spcbpt_enable_counters", "spcbpt_stream", "spcbpt_sync", "spcbpt_sync_light", "spcbpt_launch_deferred", "spcbpt_merge_deferred", "spcbpt_sync_film", "spcbpt_set_light_ahead", "spcbpt_get_pipeline_state", "spcbpt_reuse_sampler", "spcbpt_read_film", "spcbpt_debug_batch_scratch", "spcbpt_debug_read_sampling_tables", "spcbpt_lvc_import_wait", "spcbpt_kernel_time",
    "spcbpt_reset_kernel_time", "spcbpt_enable_kernel_timing", "spcbpt_trace_closest", "spcbpt_trace_any", "spcbpt_camera_splat",
    "spcbpt_set_splat_order", "spcbpt_get_splat_order", "spcbpt_read_splat_records", "spcbpt_splat_sum_host",
    "spcbpt_set_lens", "spcbpt_get_lens", "spcbpt_camera_lens_ray_host", "spcbpt_camera_splat_lens", "spcbpt_lens_sample_host", "spcbpt_debug_lens_rays",
    "spcbpt_launch_features", "spcbpt_read_features", "spcbpt_denoise", "spcbpt_denoise_params_struct_size", "spcbpt_read_denoised", "spcbpt_denoise_host",
    "spcbpt_launch_guides", "spcbpt_read_guides", "spcbpt_set_denoise_guides", "spcbpt_guide_params_struct_size", "spcbpt_guide_step_host",
    "spcbpt_set_film_moments", "spcbpt_get_film_moments", "spcbpt_read_film_moments", "spcbpt_film_moments_update_host", "spcbpt_film_error", "spcbpt_film_error_struct_size", "spcbpt_film_error_host", "spcbpt_denoise_variance", "spcbpt_denoise_variance_host",
    "spcbpt_set_film_buckets", "spcbpt_get_film_buckets", "spcbpt_read_film_buckets", "spcbpt_film_buckets_update_host", "spcbpt_robust_resolve", "spcbpt_read_robust", "spcbpt_robust_resolve_host",
    "spcbpt_display_default_params", "spcbpt_display_params_struct_size", "spcbpt_display", "spcbpt_display_image", "spcbpt_read_display", "spcbpt_display_reset", "spcbpt_display_host",
    "spcbpt_bloom_default_params", "spcbpt_bloom_params_struct_size", "spcbpt_bloom", "spcbpt_bloom_image", "spcbpt_read_bloom", "spcbpt_bloom_host",
    "spcbpt_local_tone_default_params", "spcbpt_local_tone_params_struct_size", "spcbpt_local_tone", "spcbpt_local_tone_image", "spcbpt_read_local_tone", "spcbpt_local_tone_host", "spcbpt_local_tone_math_host",
    "spcbpt_adaptive_params_struct_size", "spcbpt_adaptive_begin", "spcbpt_adaptive_end", "spcbpt_adaptive_select", "spcbpt_adaptive_set_tiles", "spcbpt_launch_adaptive",
    "spcbpt_read_adaptive", "spcbpt_get_adaptive_state", "spcbpt_adaptive_select_host",
    "spcbpt_history_capture", "spcbpt_history_reproject", "spcbpt_history_resolve", "spcbpt_history_reset", "spcbpt_read_history", "spcbpt_reproject_params_struct_size",
    "spcbpt_history_reproject_host", "spcbpt_history_resolve_host", "spcbpt_viewer_set_reproject", "spcbpt_viewer_get_reproject",
    "spcbpt_history_denoise", "spcbpt_read_history_variance", "spcbpt_history_reproject_var_host", "spcbpt_history_resolve_var_host", "spcbpt_history_denoise_host",
    "spcbpt_viewer_set_denoise", "spcbpt_viewer_get_denoise",
    "spcbpt_preprocess", "spcbpt_get_subspace", "spcbpt_scene_info", "spcbpt_set_pretrace", "spcbpt_train_records_count",
    "spcbpt_train_records_read", "spcbpt_train_records_import", "spcbpt_train_records_clear", "spcbpt_preprocess_stage",
    "spcbpt_get_gamma", "spcbpt_gltf_load", "spcbpt_scene_file_load", "spcbpt_scene_file_desc", "spcbpt_scene_file_camera",
    "spcbpt_scene_file_warnings", "spcbpt_scene_file_environment", "spcbpt_scene_file_free",
    "spcbpt_viewer_create", "spcbpt_viewer_destroy", "spcbpt_viewer_mouse_button", "spcbpt_viewer_cursor_pos", "spcbpt_viewer_scroll",
    "spcbpt_viewer_window_size", "spcbpt_viewer_iconify", "spcbpt_viewer_key", "spcbpt_viewer_set_fps", "spcbpt_viewer_set_light_ahead", "spcbpt_viewer_set_pipeline", "spcbpt_viewer_frame",
    "spcbpt_viewer_get_state", "spcbpt_viewer_alg_name",
    "spcbpt_image_load", "spcbpt_checkpoint_write", "spcbpt_checkpoint_read", "spcbpt_gamma_to_cmf", "spcbpt_checkpoint_save", "spcbpt_checkpoint_load",
]


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _source_index(source):
    """The `source` of display / bloom / local_tone: a name of DISPLAY_SOURCES, or the number itself."""
    return DISPLAY_SOURCES[source] if isinstance(source, str) else int(source)


def _image_arg(img, who):
    """An image of the caller's as the *_image calls pass it on: contiguous float32 of shape (h, w, 4)."""
    x = np.ascontiguousarray(img, dtype=np.float32)
    if x.ndim != 3 or x.shape[-1] != 4:
        raise SpcbptError(f"{who}: the image must be (h, w, 4)")
    return x


class Renderer:
    """One context per GPU (the `sutil::Scene` + `MyParams` pair of the reference driver)."""

    def __init__(self, scene: Scene, device: int = 0):
        self.lib = load_library()
        self.scene = scene
        sd, keep = scene.desc()
        h = C.c_void_p()
        if scene.mesh_lights:   # emissive meshes (spcbpt_create_lit; a scene of quads only takes the entry it always took)
            ml = scene.mesh_light_array()
            rc = self.lib.spcbpt_create_lit(C.byref(sd), ml, len(scene.mesh_lights), device, C.byref(h))
        else:
            rc = self.lib.spcbpt_create(C.byref(sd), device, C.byref(h))
        if rc != 0:
            msg = self.lib.spcbpt_last_error(None)
            raise SpcbptError(f"spcbpt_create failed ({rc}): {msg.decode() if msg else ''}")
        self.h = h
        self.width = self.height = 0
        self.lt = None

    def _chk(self, rc, what):
        if rc != 0:
            msg = self.lib.spcbpt_last_error(self.h)
            raise SpcbptError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.spcbpt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- state --------------------------------------------------------------
    def set_camera(self, eye, U, V, W):
        a = [np.ascontiguousarray(x, dtype=np.float32) for x in (eye, U, V, W)]
        self._chk(self.lib.spcbpt_set_camera(self.h, *[_fp(x) for x in a]), "set_camera")

    def set_camera_lookat(self, eye, lookat, up, fov, aspect):
        a = [np.ascontiguousarray(x, dtype=np.float32) for x in (eye, lookat, up)]
        self._chk(self.lib.spcbpt_set_camera_lookat(self.h, *[_fp(x) for x in a], fov, aspect), "set_camera_lookat")

    def resize(self, w, h):
        self._chk(self.lib.spcbpt_resize(self.h, w, h), "resize")
        self.width, self.height = w, h

    def set_lens(self, radius, focus=1.0):
        """spcbpt_set_lens: a thin lens of `radius` (world units) focused at depth `focus` (units of W; 1 = the plane through lookat).
        radius 0, the default, is the pinhole.  "SPCBPT_eye" (timed kernel), "pt" and "lt" render through it; the batched, adaptive,
        counting, sky-seeing and no_rmis forms refuse while it is set.  Survives set_camera* and resize."""
        self._chk(self.lib.spcbpt_set_lens(self.h, float(radius), float(focus)), "set_lens")

    def lens(self):
        """(radius, focus) as set; (0.0, 0.0) before the first set_lens."""
        r, f = C.c_float(), C.c_float()
        self._chk(self.lib.spcbpt_get_lens(self.h, C.byref(r), C.byref(f)), "get_lens")
        return r.value, f.value

    def lens_rays(self, subframe=0):
        """spcbpt_debug_lens_rays: (origin (h, w, 3), direction (h, w, 3)) of every pixel's lens ray of `subframe`, from the device
        function the lens kernels call."""
        out = np.zeros((self.height, self.width, 8), np.float32)
        self._chk(self.lib.spcbpt_debug_lens_rays(self.h, int(subframe), _fp(out)), "debug_lens_rays")
        return out[..., 0:3].copy(), out[..., 3:6].copy()

    def set_subspace(self, eye_tree=None, light_tree=None, q=None, cmf_gamma=None):
        if eye_tree is None and light_tree is None and q is None and cmf_gamma is None:
            self._chk(self.lib.spcbpt_set_subspace(self.h, None, 0, None, 0, None, None), "set_subspace")
            return
        et = np.ascontiguousarray(eye_tree, dtype=TREE_NODE_DTYPE)
        lt = np.ascontiguousarray(light_tree, dtype=TREE_NODE_DTYPE)
        q = np.ascontiguousarray(q, dtype=np.float32)
        g = np.ascontiguousarray(cmf_gamma, dtype=np.float32)
        assert q.size == NUM_SUBSPACE and g.size == NUM_SUBSPACE * NUM_SUBSPACE
        self._chk(self.lib.spcbpt_set_subspace(self.h, et.ctypes.data, et.shape[0], lt.ctypes.data, lt.shape[0],
                                               q.ctypes.data, g.ctypes.data), "set_subspace")

    def get_subspace(self, cap=1 << 20):
        et = np.zeros(cap, dtype=TREE_NODE_DTYPE)
        lt = np.zeros(cap, dtype=TREE_NODE_DTYPE)
        q = np.zeros(NUM_SUBSPACE, dtype=np.float32)
        g = np.zeros(NUM_SUBSPACE * NUM_SUBSPACE, dtype=np.float32)
        ne, nl = C.c_int(), C.c_int()
        self._chk(self.lib.spcbpt_get_subspace(self.h, et.ctypes.data, C.byref(ne), cap, lt.ctypes.data, C.byref(nl), cap,
                                               q.ctypes.data, g.ctypes.data), "get_subspace")
        return et[:ne.value].copy(), lt[:nl.value].copy(), q, g.reshape(NUM_SUBSPACE, NUM_SUBSPACE)

    def set_light_trace(self, num_core, core_padding, m_per_core, core_begin=0, core_count=0, decorrelate=None):
        if decorrelate is None:
            decorrelate = m_per_core == 1   # one path per lane: see spcbpt_light_trace_params in include/spcbpt.h
        p = LightTraceParams(num_core, core_padding, m_per_core, core_begin, core_count, int(decorrelate))
        self._chk(self.lib.spcbpt_set_light_trace(self.h, C.byref(p)), "set_light_trace")
        self.lt = p

    # -- launches -----------------------------------------------------------
    def launch(self, name: str, frame: int, rows=None):
        """spcbpt_launch: "light trace", "pt", "SPCBPT_eye", "SPCBPT_no_rmis", "pretrace", or "lt" -- light tracing, the light-vertex
        cache of the last built sampler splatted onto the film (no environment map; float atomics, so not bit-reproducible, unless
        set_splat_order(SPLAT_ORDERED) has been called)."""
        r0, r1, rs = rows if rows is not None else (0, self.height, 1)
        self._chk(self.lib.spcbpt_launch(self.h, name.encode(), frame, r0, r1, rs), f"launch({name})")

    def set_splat_order(self, mode):
        """spcbpt_set_splat_order: SPLAT_ATOMIC (0, the default) or SPLAT_ORDERED (1): "lt" sums every pixel's contributions in
        ascending cache order, so its film is the same bits on every run (32 B per cache vertex and render stream, a radix sort per
        launch).  True / False select ordered / atomic."""
        self._chk(self.lib.spcbpt_set_splat_order(self.h, int(mode)), "set_splat_order")

    def splat_order(self) -> int:
        v = C.c_int32()
        self._chk(self.lib.spcbpt_get_splat_order(self.h, C.byref(v)), "get_splat_order")
        return v.value

    def read_splat_records(self, capacity=None):
        """spcbpt_read_splat_records: (rgb (n, 3) float32, pixel (n,) int32) of the last ordered "lt" launch, one entry per vertex
        of the cache it read, in cache order; pixel = y * width + x, or -1 where the vertex added nothing."""
        n = C.c_int()
        if capacity is None:   # ask for the count first (no buffers: SPCBPT_ERR_CAPACITY with the count set, unless it is 0)
            rc = self.lib.spcbpt_read_splat_records(self.h, None, None, 0, C.byref(n))
            if rc not in (0, -6):
                self._chk(rc, "read_splat_records")
            capacity = n.value
        rgb = np.zeros((max(capacity, 1), 3), np.float32)
        pixel = np.full(max(capacity, 1), -1, np.int32)
        self._chk(self.lib.spcbpt_read_splat_records(self.h, _fp(rgb), pixel.ctypes.data_as(C.POINTER(C.c_int32)), int(capacity), C.byref(n)), "read_splat_records")
        return rgb[:n.value].copy(), pixel[:n.value].copy()

    def launch_features(self, subframe: int, rows=None):
        """spcbpt_launch_features: the first hit of the film's primary ray of `subframe` (albedo + coverage, geometric normal + depth)
        merged into the feature buffers as a running mean over the subframes; rows as in launch()."""
        r0, r1, rs = rows if rows is not None else (0, self.height, 1)
        self._chk(self.lib.spcbpt_launch_features(self.h, int(subframe), r0, r1, rs), "launch_features")

    def launch_guides(self, subframe: int, rows=None, max_bounces=GUIDE_MAX_BOUNCES, roughness_max=GUIDE_ROUGHNESS_MAX, metallic_min=GUIDE_METALLIC_MIN):
        """spcbpt_launch_guides: launch_features' ray followed through up to `max_bounces` (0 .. 8) mirror-like surfaces (roughness <=
        roughness_max and metallic >= metallic_min) to the first surface that is not one; albedo x the mirrors' tints + coverage, and
        the normal + path length unfolded through the mirrors, merged into the guide planes as running means; rows as in launch()."""
        r0, r1, rs = rows if rows is not None else (0, self.height, 1)
        p = GuideParams(int(max_bounces), float(roughness_max), float(metallic_min))
        self._chk(self.lib.spcbpt_launch_guides(self.h, int(subframe), r0, r1, rs, C.byref(p)), "launch_guides")

    def set_denoise_guides(self, which):
        """spcbpt_set_denoise_guides: "first_hit" (the default) or "reflected" -- the planes denoise() and denoise_variance() take albedo
        and normal + depth from (launch_guides first for "reflected").  The history calls and adaptive sampling keep the first hit."""
        self._chk(self.lib.spcbpt_set_denoise_guides(self.h, DENOISE_GUIDES[which] if isinstance(which, str) else int(which)), "set_denoise_guides")

    def denoise(self, iterations=5, sigma_c=0.0, sigma_n=0.0, sigma_x=0.0):
        """spcbpt_denoise: the edge-avoiding a-trous filter on the film divided by the first-hit albedo, guided by the feature buffers
        (launch_features first).  A sigma <= 0 takes its default; sigma_x is a length in scene units.  The film is not touched."""
        p = DenoiseParams(int(iterations), float(sigma_c), float(sigma_n), float(sigma_x))
        self._chk(self.lib.spcbpt_denoise(self.h, C.byref(p)), "denoise")

    def denoise_variance(self, iterations=5, sigma_v=0.0, sigma_n=0.0, sigma_x=0.0):
        """spcbpt_denoise_variance: the a-trous filter with its colour weight measured in the pixel's own standard error (the film's
        moments: set_film_moments(True) before rendering; launch_features first), so that it narrows as the film converges.  A sigma
        <= 0 takes its default.  The result is read with read_denoised(); the film is not touched."""
        p = DenoiseParams(int(iterations), float(sigma_v), float(sigma_n), float(sigma_x))
        self._chk(self.lib.spcbpt_denoise_variance(self.h, C.byref(p)), "denoise_variance")

    def set_film_moments(self, on: bool):
        """spcbpt_set_film_moments: keep the per-pixel second moment of the film (16 B per pixel, one small kernel per merge)."""
        self._chk(self.lib.spcbpt_set_film_moments(self.h, 1 if on else 0), "set_film_moments")

    def film_moments(self) -> bool:
        v = C.c_int32()
        self._chk(self.lib.spcbpt_get_film_moments(self.h, C.byref(v)), "get_film_moments")
        return bool(v.value)

    def film_error(self):
        """spcbpt_film_error: {"pixels", "mean", "max"} of the relative standard error over the pixels with at least two samples."""
        out = FilmErrorStats()
        self._chk(self.lib.spcbpt_film_error(self.h, C.byref(out)), "film_error")
        return out.as_dict()

    # ---- bucket film and robust resolve (spcbpt_set_film_buckets, spcbpt_robust_resolve)
    def set_film_buckets(self, k: int):
        """spcbpt_set_film_buckets: keep K per-pixel bucket means of the film (16 K B per pixel, one small kernel per merge); K = 0
        switches off, 3 .. 32 on."""
        self._chk(self.lib.spcbpt_set_film_buckets(self.h, int(k)), "set_film_buckets")

    def film_buckets(self) -> int:
        v = C.c_int32()
        self._chk(self.lib.spcbpt_get_film_buckets(self.h, C.byref(v)), "get_film_buckets")
        return int(v.value)

    def read_film_buckets(self):
        """(K, h, w, 4) float32: (mean_r, mean_g, mean_b, n) per bucket and pixel (spcbpt_read_film_buckets)."""
        k = self.film_buckets()
        self.image_size()
        out = np.zeros((max(k, 1), self.height, self.width, 4), dtype=np.float32)
        self._chk(self.lib.spcbpt_read_film_buckets(self.h, out.ctypes.data), "read_film_buckets")
        return out

    def robust_resolve(self, strength=1.0):
        """spcbpt_robust_resolve: the median-of-means image of the bucket film, trimmed by `strength` in [0, 8] times the Gini
        coefficient of the pixel's bucket luminances (0 is the film's mean).  Read with read_robust(); the film is not touched."""
        self._chk(self.lib.spcbpt_robust_resolve(self.h, float(strength)), "robust_resolve")

    def read_robust(self):
        """(rgbw float32, rgba8): the result of the last robust_resolve() -- w the number of buckets kept -- and its tone-mapped frame."""
        self.image_size()
        d = np.zeros((self.height, self.width, 4), dtype=np.float32)
        f = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self._chk(self.lib.spcbpt_read_robust(self.h, d.ctypes.data, f.ctypes.data), "read_robust")
        return d, f

    # ---- display transform (spcbpt_display*): exposure, histogram auto-exposure, tone operators -- an RGBA8 plane of its own
    def display(self, source="film", **params):
        """spcbpt_display: one of the context's linear images -- every source of DISPLAY_SOURCES: "film", "denoised", "robust", "history",
        the bloom plane ("bloom") or the local tone plane ("local") -- times 2^EV through a tone operator into the display plane.
        Parameters as display_params takes them: op="film" | "reinhard" | "aces" | "linear", ev=..., auto=True (EV from the image's
        histogram, adapted on the device), histogram=True, key=..., ...  Read with read_display()."""
        src, p = _source_index(source), display_params(**params)
        self._chk(self.lib.spcbpt_display(self.h, src, C.byref(p)), "display")

    def display_image(self, img, **params):
        """spcbpt_display_image: the same pass on an (h, w, 4) float32 image of the caller's, any size."""
        x, p = _image_arg(img, "display_image"), display_params(**params)
        self._chk(self.lib.spcbpt_display_image(self.h, _fp(x), x.shape[1], x.shape[0], C.byref(p)), "display_image")

    def _display_size(self):
        w, h = C.c_int32(), C.c_int32()
        self._chk(self.lib.spcbpt_read_display(self.h, None, None, None, C.byref(w), C.byref(h)), "read_display")
        return int(w.value), int(h.value)

    def read_display(self):
        """(rgba8 (h, w, 4) uint8, ev): what the last display() / display_image() wrote and the EV it applied."""
        w, h = self._display_size()
        out = np.zeros((h, w, 4), dtype=np.uint8)
        ev = C.c_float()
        self._chk(self.lib.spcbpt_read_display(self.h, out.ctypes.data, None, C.byref(ev), None, None), "read_display")
        return out, float(ev.value)

    def read_display_histogram(self):
        """(258,) uint32: the luminance histogram of the last display call's image -- 256 bins over [2^-16, 2^16), eight per octave,
        then `dark` and `bright`.  Needs auto=True or histogram=True in that call."""
        hist = np.zeros(DISPLAY_COUNTERS, dtype=np.uint32)
        self._chk(self.lib.spcbpt_read_display(self.h, None, hist.ctypes.data, None, None, None), "read_display")
        return hist

    def display_reset(self):
        """spcbpt_display_reset: forget the previous EV (the next auto call jumps to its target)."""
        self._chk(self.lib.spcbpt_display_reset(self.h), "display_reset")

    # ---- bloom (spcbpt_bloom*): a multi-scale glare ahead of the display transform -- a float4 plane of its own
    def bloom(self, source="film", **params):
        """spcbpt_bloom: one of the context's film-sized linear images -- "film", "denoised", "robust" or "history"; the "bloom" and
        "local" planes of DISPLAY_SOURCES are no source of this stage -- with the share `strength` of its light above `threshold`
        spread over `levels` scales, into the bloom plane.  Parameters as bloom_params takes them.  Read with read_bloom(); show with
        display("bloom", ...)."""
        src, p = _source_index(source), bloom_params(**params)
        self._chk(self.lib.spcbpt_bloom(self.h, src, C.byref(p)), "bloom")

    def bloom_image(self, img, **params):
        """spcbpt_bloom_image: the same stage on an (h, w, 4) float32 image of the caller's, any size."""
        x, p = _image_arg(img, "bloom_image"), bloom_params(**params)
        self._chk(self.lib.spcbpt_bloom_image(self.h, _fp(x), x.shape[1], x.shape[0], C.byref(p)), "bloom_image")

    def _read_plane(self, fn, who):
        """A float4 plane at a size of its own (spcbpt_read_bloom, spcbpt_read_local_tone): the size first, then the plane."""
        w, h = C.c_int32(), C.c_int32()
        self._chk(fn(self.h, None, C.byref(w), C.byref(h)), who)
        out = np.zeros((int(h.value), int(w.value), 4), dtype=np.float32)
        self._chk(fn(self.h, out.ctypes.data, None, None), who)
        return out

    def read_bloom(self):
        """(h, w, 4) float32: the plane the last bloom() / bloom_image() wrote, at that call's image size."""
        return self._read_plane(self.lib.spcbpt_read_bloom, "read_bloom")

    # ---- local tone mapping (spcbpt_local_tone*): base / detail through a bilateral grid -- a float4 plane of its own
    def local_tone(self, source="film", **params):
        """spcbpt_local_tone: one of the context's linear images -- "film", "denoised", "robust", "history" or the bloom plane ("bloom");
        the "local" plane of DISPLAY_SOURCES is no source of this stage -- with its large-scale luminance range compressed by `compress`
        about `anchor` and its local contrast scaled by `detail`, into the local tone plane.  Parameters as local_tone_params takes
        them.  Read with read_local_tone(); show with display("local", ...)."""
        src, p = _source_index(source), local_tone_params(**params)
        self._chk(self.lib.spcbpt_local_tone(self.h, src, C.byref(p)), "local_tone")

    def local_tone_image(self, img, **params):
        """spcbpt_local_tone_image: the same stage on an (h, w, 4) float32 image of the caller's, any size."""
        x, p = _image_arg(img, "local_tone_image"), local_tone_params(**params)
        self._chk(self.lib.spcbpt_local_tone_image(self.h, _fp(x), x.shape[1], x.shape[0], C.byref(p)), "local_tone_image")

    def read_local_tone(self):
        """(h, w, 4) float32: the plane the last local_tone() / local_tone_image() wrote, at that call's image size."""
        return self._read_plane(self.lib.spcbpt_read_local_tone, "read_local_tone")

    # ---- adaptive sampling (spcbpt_adaptive_*): tiles are 8x8 pixels of the whole film, numbered x-major
    def adaptive_begin(self, frames: int):
        """spcbpt_adaptive_begin: the film holds the uniform subframes 0 .. frames - 1; from here on it is merged tile by tile.  Needs the
        film's moments (set_film_moments(True) before the frames were rendered)."""
        self._chk(self.lib.spcbpt_adaptive_begin(self.h, int(frames)), "adaptive_begin")

    def adaptive_end(self):
        """spcbpt_adaptive_end: back to ordinary launches; the film stays as it is."""
        self._chk(self.lib.spcbpt_adaptive_end(self.h), "adaptive_end")

    def adaptive_select(self, target_error, min_samples=0, max_samples=0) -> int:
        """spcbpt_adaptive_select: lists the tiles below max_samples that have fewer than max(min_samples, 2) samples, no pixel with two
        samples, or a mean relative standard error above target_error.  Returns the list's length."""
        p = AdaptiveParams(float(target_error), int(min_samples), int(max_samples))
        n = C.c_int(0)
        self._chk(self.lib.spcbpt_adaptive_select(self.h, C.byref(p), C.byref(n)), "adaptive_select")
        return int(n.value)

    def adaptive_set_tiles(self, tiles):
        """spcbpt_adaptive_set_tiles: imposes a tile list (strictly ascending, in range; may be empty)."""
        t = np.asarray(tiles)
        if t.size and (t.min() < 0 or t.max() > 0xffffffff):
            raise SpcbptError("adaptive_set_tiles: tile indices must fit 32 unsigned bits")
        t = np.ascontiguousarray(t, dtype=np.uint32).reshape(-1)
        self._chk(self.lib.spcbpt_adaptive_set_tiles(self.h, t.ctypes.data if t.size else None, int(t.size)), "adaptive_set_tiles")

    def launch_adaptive(self, alg: str = "SPCBPT_eye"):
        """spcbpt_launch_adaptive: one sample for every pixel of every listed tile, each tile at its own sample index, merged into the
        listed tiles only.  After a light pass and a sampler build, like launch("SPCBPT_eye", ...)."""
        self._chk(self.lib.spcbpt_launch_adaptive(self.h, alg.encode()), "launch_adaptive")

    def adaptive_state(self):
        """spcbpt_get_adaptive_state: {"active", "tiles_x", "tiles_y", "n_listed"}; never waits."""
        a, tx, ty, n = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.lib.spcbpt_get_adaptive_state(self.h, C.byref(a), C.byref(tx), C.byref(ty), C.byref(n)), "get_adaptive_state")
        return {"active": bool(a.value), "tiles_x": int(tx.value), "tiles_y": int(ty.value), "n_listed": int(n.value)}

    def read_adaptive(self):
        """spcbpt_read_adaptive: {"samples": (tiles_y, tiles_x) uint32, "error": (tiles_y, tiles_x) float32 of the last select,
        "tiles": the current list}."""
        st = self.adaptive_state()
        ty, tx = st["tiles_y"], st["tiles_x"]
        samples = np.zeros((ty, tx), dtype=np.uint32)
        error = np.zeros((ty, tx), dtype=np.float32)
        tiles = np.zeros(max(1, tx * ty), dtype=np.uint32)
        n = C.c_int(0)
        self._chk(self.lib.spcbpt_read_adaptive(self.h, samples.ctypes.data, error.ctypes.data, tiles.ctypes.data, int(tiles.size), C.byref(n)), "read_adaptive")
        return {"samples": samples, "error": error, "tiles": tiles[:n.value].copy()}

    def launch_light_batch(self, first_frame, n):
        """The light passes of launch frames first_frame .. first_frame + n - 1 as one persistent launch (spcbpt_launch_light_batch)."""
        self._chk(self.lib.spcbpt_launch_light_batch(self.h, first_frame, n), "launch_light_batch")

    def launch_eye_batch(self, subframes, rows=None):
        """One persistent eye kernel over the samplers of the last len(subframes) build_sampler calls (spcbpt_launch_eye_batch)."""
        sf = (C.c_uint32 * len(subframes))(*[int(v) for v in subframes])
        r0, r1, rs = rows if rows is not None else (0, self.height, 1)
        self._chk(self.lib.spcbpt_launch_eye_batch(self.h, len(subframes), sf, r0, r1, rs), "launch_eye_batch")

    def launch_eye_batch_film(self, subframes, rows=None):
        """launch_eye_batch whose merge keeps the film's second moment and fills its buckets, whichever are on
        (spcbpt_launch_eye_batch_film): the film, the moments and the buckets of len(subframes) per-frame launches."""
        sf = (C.c_uint32 * len(subframes))(*[int(v) for v in subframes])
        r0, r1, rs = rows if rows is not None else (0, self.height, 1)
        self._chk(self.lib.spcbpt_launch_eye_batch_film(self.h, len(subframes), sf, r0, r1, rs), "launch_eye_batch_film")

    def build_sampler(self):
        self._chk(self.lib.spcbpt_build_sampler(self.h), "build_sampler")

    def build_sampler_batch(self, n: int):
        """n build_sampler calls (the n oldest queued light passes) as one set of four launches (spcbpt_build_sampler_batch)."""
        self._chk(self.lib.spcbpt_build_sampler_batch(self.h, int(n)), "build_sampler_batch")

    def sync(self):
        self._chk(self.lib.spcbpt_sync(self.h), "sync")

    def launch_deferred(self, alg: str, subframe: int, rows=None):
        r0, r1, rs = rows if rows is not None else (0, self.height, 1)
        self._chk(self.lib.spcbpt_launch_deferred(self.h, alg.encode(), int(subframe), r0, r1, rs), "launch_deferred")

    def merge_deferred(self, keep: bool):
        self._chk(self.lib.spcbpt_merge_deferred(self.h, 1 if keep else 0), "merge_deferred")

    def sync_film(self):
        self._chk(self.lib.spcbpt_sync_film(self.h), "sync_film")

    def preprocess(self, target_paths=2_000_000, target_q_paths=2_000_000, train=True):
        self._chk(self.lib.spcbpt_preprocess(self.h, target_paths, target_q_paths, int(train)), "preprocess")

    def set_pretrace(self, num_core=10000, padding=10):
        self._chk(self.lib.spcbpt_set_pretrace(self.h, num_core, padding), "set_pretrace")

    def preprocess_stage(self, stage: int, arg: int = 0):
        self._chk(self.lib.spcbpt_preprocess_stage(self.h, stage, arg), f"preprocess_stage({stage})")

    def train_records(self):
        a, b = C.c_int(), C.c_int()
        self._chk(self.lib.spcbpt_train_records_count(self.h, C.byref(a), C.byref(b)), "train_records_count")
        paths = np.zeros(a.value, dtype=PRETRACE_PATH_DTYPE)
        nodes = np.zeros(b.value, dtype=PRETRACE_NODE_DTYPE)
        if a.value:
            self._chk(self.lib.spcbpt_train_records_read(self.h, paths.ctypes.data, a.value, nodes.ctypes.data, max(b.value, 1)),
                      "train_records_read")
        return paths, nodes

    def train_records_import(self, paths, nodes):
        pa = np.ascontiguousarray(paths, dtype=PRETRACE_PATH_DTYPE)
        no = np.ascontiguousarray(nodes, dtype=PRETRACE_NODE_DTYPE)
        self._chk(self.lib.spcbpt_train_records_import(self.h, pa.ctypes.data, pa.shape[0], no.ctypes.data, no.shape[0]),
                  "train_records_import")

    def train_records_clear(self):
        self._chk(self.lib.spcbpt_train_records_clear(self.h), "train_records_clear")

    def checkpoint_save(self, directory: str):
        """tree_eye.txt, tree_light.txt, Q.txt, E.txt in the reference's formats (needs a preprocessing run for Gamma)."""
        self._chk(self.lib.spcbpt_checkpoint_save(self.h, os.fsencode(directory)), "checkpoint_save")

    def checkpoint_load(self, directory: str):
        self._chk(self.lib.spcbpt_checkpoint_load(self.h, os.fsencode(directory)), "checkpoint_load")

    def get_gamma(self):
        g = np.zeros((NUM_SUBSPACE, NUM_SUBSPACE), dtype=np.float32)
        self._chk(self.lib.spcbpt_get_gamma(self.h, g.ctypes.data), "get_gamma")
        return g

    # -- readback -----------------------------------------------------------
    def image_size(self):
        """(width, height) as the library holds them (the viewer resizes the context itself)."""
        w, h = C.c_int32(), C.c_int32()
        self._chk(self.lib.spcbpt_image_size(self.h, C.byref(w), C.byref(h)), "image_size")
        self.width, self.height = int(w.value), int(h.value)
        return self.width, self.height

    def read_accum(self):
        self.image_size()
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        self._chk(self.lib.spcbpt_read_accum(self.h, out.ctypes.data), "read_accum")
        return out

    def read_frame(self):
        self.image_size()
        out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self._chk(self.lib.spcbpt_read_frame(self.h, out.ctypes.data), "read_frame")
        return out

    def read_features(self):
        """(albedo, normal_depth): (h, w, 4) float32 each -- base colour + coverage, normal + depth (spcbpt_read_features)."""
        self.image_size()
        a = np.zeros((self.height, self.width, 4), dtype=np.float32)
        n = np.zeros((self.height, self.width, 4), dtype=np.float32)
        self._chk(self.lib.spcbpt_read_features(self.h, a.ctypes.data, n.ctypes.data), "read_features")
        return a, n

    def read_guides(self):
        """(albedo, normal_depth): (h, w, 4) float32 each -- the reflected guide planes in read_features' layout (spcbpt_read_guides)."""
        self.image_size()
        a = np.zeros((self.height, self.width, 4), dtype=np.float32)
        n = np.zeros((self.height, self.width, 4), dtype=np.float32)
        self._chk(self.lib.spcbpt_read_guides(self.h, a.ctypes.data, n.ctypes.data), "read_guides")
        return a, n

    def read_film_moments(self):
        """(h, w, 4) float32: (M2_r, M2_g, M2_b, n) per pixel (spcbpt_read_film_moments); variance of the mean = M2 / (n (n - 1))."""
        self.image_size()
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        self._chk(self.lib.spcbpt_read_film_moments(self.h, out.ctypes.data), "read_film_moments")
        return out

    def history_capture(self, frames):
        """spcbpt_history_capture: keep what history_resolve(frames) would show, with the feature plane and the camera, as the
        history of the next reprojection.  Needs launch_features since the last resize."""
        self._chk(self.lib.spcbpt_history_capture(self.h, int(frames)), "history_capture")

    def history_reproject(self, sigma_n=0.0, sigma_x=0.0, max_history=0.0):
        """spcbpt_history_reproject: the captured history carried into the current view through the first-hit depth (the prior).
        Needs launch_features(0) of the current view; a parameter <= 0 takes its default."""
        p = ReprojectParams(float(sigma_n), float(sigma_x), float(max_history))
        self._chk(self.lib.spcbpt_history_reproject(self.h, C.byref(p)), "history_reproject")

    def history_resolve(self, frames):
        """spcbpt_history_resolve: the prior (if one is live) blended with the film's mean of `frames` frames; read with read_history()."""
        self._chk(self.lib.spcbpt_history_resolve(self.h, int(frames)), "history_resolve")

    def history_denoise(self, iterations=5, sigma_v=0.0, sigma_n=0.0, sigma_x=0.0):
        """spcbpt_history_denoise: denoise_variance's filter on the resolved image, guided by the variance the history carries (the
        moments on from the capture on: set_film_moments(True); launch_features and history_resolve first).  A sigma <= 0 takes its
        default.  The result is read with read_denoised(); film and history planes are not touched."""
        p = DenoiseParams(int(iterations), float(sigma_v), float(sigma_n), float(sigma_x))
        self._chk(self.lib.spcbpt_history_denoise(self.h, C.byref(p)), "history_denoise")

    def read_history_variance(self, resolved=True, prior=False, history=False):
        """spcbpt_read_history_variance: a dict of the (h, w, 4) float32 variance planes asked for -- (V_r, V_g, V_b, 0), the variance of
        the mean -- of the "resolved" image, the "prior", the captured "history".  SpcbptError (-5) for a plane that is not valid."""
        w, h = self.image_size()
        want = {"resolved": resolved, "prior": prior, "history": history}
        out = {k: np.zeros((h, w, 4), dtype=np.float32) for k, on in want.items() if on}
        self._chk(self.lib.spcbpt_read_history_variance(self.h, *[out[k].ctypes.data if k in out else None for k in want]), "read_history_variance")
        return out

    def history_reset(self):
        self._chk(self.lib.spcbpt_history_reset(self.h), "history_reset")

    def read_history(self, resolved=True, frame=True, prior=False, history=False):
        """spcbpt_read_history: a dict of the planes asked for -- "resolved" (h, w, 4) float32 and its tone-mapped "frame" (h, w, 4) uint8,
        the "prior" (rgb, m), the captured "history" (rgb, n).  SpcbptError (-5) for a plane that does not exist yet."""
        self.image_size()
        want = {"resolved": (resolved, np.float32), "frame": (frame, np.uint8), "prior": (prior, np.float32), "history": (history, np.float32)}
        out = {k: np.zeros((self.height, self.width, 4), dtype=t) for k, (on, t) in want.items() if on}
        self._chk(self.lib.spcbpt_read_history(self.h, *[out[k].ctypes.data if k in out else None for k in want]), "read_history")
        return out

    def read_denoised(self):
        """(rgba float32, rgba8): the result of the last denoise() and its tone-mapped frame (spcbpt_read_denoised)."""
        self.image_size()
        d = np.zeros((self.height, self.width, 4), dtype=np.float32)
        f = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self._chk(self.lib.spcbpt_read_denoised(self.h, d.ctypes.data, f.ctypes.data), "read_denoised")
        return d, f

    def clear_accum(self):
        self._chk(self.lib.spcbpt_clear_accum(self.h), "clear_accum")

    def read_film(self, accum=True, frame=True):
        """(accum, frame) as of the last queued film merge, without waiting for launches queued behind it (spcbpt_read_film)."""
        self.image_size()
        a = np.zeros((self.height, self.width, 4), dtype=np.float32) if accum else None
        f = np.zeros((self.height, self.width, 4), dtype=np.uint8) if frame else None
        self._chk(self.lib.spcbpt_read_film(self.h, a.ctypes.data if accum else None, f.ctypes.data if frame else None), "read_film")
        return a, f

    def pipeline_state(self):
        v = [C.c_int32() for _ in range(4)]
        self._chk(self.lib.spcbpt_get_pipeline_state(self.h, *[C.byref(x) for x in v]), "get_pipeline_state")
        return dict(zip(("light_ahead", "pending_passes", "sampler_intact", "deferred"), (int(x.value) for x in v)))

    def reuse_sampler(self):
        self._chk(self.lib.spcbpt_reuse_sampler(self.h), "reuse_sampler")

    def batch_scratch(self):
        b, f, k = C.c_int64(), C.c_int32(), C.c_int32()
        self._chk(self.lib.spcbpt_debug_batch_scratch(self.h, C.byref(b), C.byref(f), C.byref(k)), "debug_batch_scratch")
        return {"bytes": int(b.value), "frames": int(f.value), "fallbacks": int(k.value)}

    def sampling_tables(self, vertex_count):
        """(guide2, guide1, gamma_q): the tables the eye kernel samples through (spcbpt_debug_read_sampling_tables)."""
        g2 = np.zeros(max(vertex_count, 1), dtype=np.uint32)
        g1 = np.zeros((NUM_SUBSPACE, 1024), dtype=np.uint16)
        gq = np.zeros((NUM_SUBSPACE, NUM_SUBSPACE), dtype=np.float32)
        self._chk(self.lib.spcbpt_debug_read_sampling_tables(self.h, g2.ctypes.data if vertex_count > 0 else None, len(g2), g1.ctypes.data, gq.ctypes.data),
                  "debug_read_sampling_tables")
        return g2[:vertex_count], g1, gq

    def lvc_read(self, capacity=None):
        if capacity is None:
            capacity = self.lt.num_core * self.lt.core_padding if self.lt else 1 << 22
        out = np.zeros(capacity, dtype=LIGHT_VERTEX_DTYPE)
        n = C.c_int()
        self._chk(self.lib.spcbpt_lvc_read(self.h, out.ctypes.data, capacity, C.byref(n)), "lvc_read")
        return out[:n.value].copy()

    def lvc_import(self, verts: np.ndarray):
        v = np.ascontiguousarray(verts, dtype=LIGHT_VERTEX_DTYPE)
        self._chk(self.lib.spcbpt_lvc_import(self.h, v.ctypes.data, v.shape[0], 0), "lvc_import")

    def lvc_import_device(self, d_ptr: int, count: int):
        self._chk(self.lib.spcbpt_lvc_import(self.h, C.c_void_p(d_ptr), count, 1), "lvc_import")

    def set_environment(self, rgba, center=None, radius=0.0):
        """The environment map as one more light (spcbpt_set_environment): rgba = (h, w, 4) float32 as the .hdr stores it (row 0 = top)."""
        a = np.ascontiguousarray(rgba, dtype=np.float32)
        assert a.ndim == 3 and a.shape[2] == 4
        c3 = None if center is None else np.ascontiguousarray(center, dtype=np.float32)
        self._chk(self.lib.spcbpt_set_environment(self.h, a.ctypes.data, a.shape[1], a.shape[0], None if c3 is None else c3.ctypes.data, float(radius)), "set_environment")

    def environment(self):
        w, h, n = C.c_int(), C.c_int(), C.c_int()
        c3 = np.zeros(3, np.float32)
        r = C.c_float()
        self._chk(self.lib.spcbpt_get_environment(self.h, C.byref(w), C.byref(h), _fp(c3), C.byref(r), C.byref(n)), "get_environment")
        f = C.c_int()
        self._chk(self.lib.spcbpt_get_environment_mode(self.h, C.byref(f)), "get_environment_mode")
        return dict(width=w.value, height=h.value, center=c3, radius=r.value, n_lights=n.value, flags=f.value)

    def set_environment_mode(self, flags: int):
        """spcbpt_set_environment_mode: ENV_EYE_SEES_SKY (1) = escaped "SPCBPT_eye" eye sub-paths see the sky (rmis::light_hit_env,
        corrected sign); ENV_PT_SKY_SHADOW_ALONG_DIR (2) = "pt"'s sky shadow ray ends at P + d 2r.  0 = upstream's behaviour."""
        self._chk(self.lib.spcbpt_set_environment_mode(self.h, int(flags)), "set_environment_mode")

    def lvc_set_capacity(self, vertices: int):
        """Vertices per buffer set, fixed by hand (0 = sized from a probe pass: spcbpt_lvc_set_capacity)."""
        self._chk(self.lib.spcbpt_lvc_set_capacity(self.h, int(vertices)), "lvc_set_capacity")

    def lvc_capacity(self):
        """(vertices per buffer set, number of sets) as allocated now."""
        v, n = C.c_int(), C.c_int()
        self._chk(self.lib.spcbpt_lvc_get_capacity(self.h, C.byref(v), C.byref(n)), "lvc_get_capacity")
        return v.value, n.value

    def lvc_export(self):
        dv, dc, cap = C.c_void_p(), C.c_void_p(), C.c_int()
        self._chk(self.lib.spcbpt_lvc_export(self.h, C.byref(dv), C.byref(dc), C.byref(cap)), "lvc_export")
        return dv.value, dc.value, cap.value

    def sampler_read(self, capacity=None):
        if capacity is None:
            capacity = self.lt.num_core * self.lt.core_padding if self.lt else 1 << 22
        sub = np.zeros(NUM_SUBSPACE, dtype=SUBSPACE_DTYPE)
        cmfs = np.zeros(capacity, dtype=np.float32)
        jump = np.zeros(capacity, dtype=np.int32)
        vc, pc = C.c_int(), C.c_int()
        self._chk(self.lib.spcbpt_sampler_read(self.h, sub.ctypes.data, cmfs.ctypes.data, jump.ctypes.data, capacity,
                                               C.byref(vc), C.byref(pc)), "sampler_read")
        return sub, cmfs[:vc.value].copy(), jump[:vc.value].copy(), vc.value, pc.value

    def accum_device_ptr(self):
        p = C.c_void_p()
        self._chk(self.lib.spcbpt_accum_device_ptr(self.h, C.byref(p)), "accum_device_ptr")
        return p.value

    def set_light_ahead(self, on: bool):
        """Light passes may be launched one frame ahead of their exchange / sampler build (see spcbpt_set_light_ahead)."""
        self._chk(self.lib.spcbpt_set_light_ahead(self.h, int(on)), "set_light_ahead")

    def lvc_import_wait(self):
        """Before overwriting one of two alternating device staging buffers of lvc_import_device (spcbpt_lvc_import_wait)."""
        self._chk(self.lib.spcbpt_lvc_import_wait(self.h), "lvc_import_wait")

    def sync_light(self):
        self._chk(self.lib.spcbpt_sync_light(self.h), "sync_light")

    def stream(self):
        p = C.c_void_p()
        self._chk(self.lib.spcbpt_stream(self.h, C.byref(p)), "stream")
        return p.value or 0

    # -- instrumentation ----------------------------------------------------
    def counters(self):
        c = Counters()
        self._chk(self.lib.spcbpt_get_counters(self.h, C.byref(c)), "get_counters")
        return c.as_dict()

    def phase_clocks(self):
        out = (C.c_uint64 * 19)()
        self._chk(self.lib.spcbpt_debug_phase_clocks(self.h, out), "debug_phase_clocks")
        return dict(zip(("regen", "closest", "shade", "shadow_pool", "connect", "node_slots", "node_lanes", "tri_slots", "tri_lanes", "sample_lane_clocks",
                         "wave_start_min", "wave_end_max", "wave_end_sum", "waves", "tail_slots", "tail_closest_lanes", "tail_shadow_lanes", "job_slots", "job_lanes"),
                        [int(v) for v in out]))

    def set_connection_sampler(self, mode: int):
        """0 = the subspace sampler (sampleFirstStage + sampleSecondStage), 1 = uniformSample ("plain BDPT", cuProg.h:283-289)"""
        self._chk(self.lib.spcbpt_set_connection_sampler(self.h, int(mode)), "set_connection_sampler")

    def unit(self, op: int, records: np.ndarray, out_words: int, aux: Optional[np.ndarray] = None) -> np.ndarray:
        """spcbpt_debug_unit: `records` is an (n, in_words) array of 32-bit words (any 4-byte dtype / structured dtype of that
        size); returns an (n, out_words) uint32 array."""
        a = np.ascontiguousarray(records)
        n = a.shape[0]
        in_words = a.dtype.itemsize // 4 if a.ndim == 1 else a.shape[1] * a.dtype.itemsize // 4
        out = np.zeros((n, out_words), np.uint32)
        ax = None if aux is None else np.ascontiguousarray(aux, dtype=np.float32)
        self._chk(self.lib.spcbpt_debug_unit(self.h, int(op), C.c_void_p(a.ctypes.data), in_words, C.c_void_p(out.ctypes.data), out_words, n,
                                             None if ax is None else C.c_void_p(ax.ctypes.data), 0 if ax is None else int(ax.size)), "debug_unit")
        return out

    def spill_arm(self):
        self._chk(self.lib.spcbpt_debug_spill_arm(self.h), "debug_spill_arm")

    def spill_count(self):
        """(words of the HBM traversal-stack spill areas written since spill_arm(), spill entries per thread)"""
        n, e = C.c_uint64(), C.c_int32()
        self._chk(self.lib.spcbpt_debug_spill_count(self.h, C.byref(n), C.byref(e)), "debug_spill_count")
        return int(n.value), int(e.value)

    def reset_counters(self):
        self._chk(self.lib.spcbpt_reset_counters(self.h), "reset_counters")

    def enable_counters(self, on: bool):
        self._chk(self.lib.spcbpt_enable_counters(self.h, int(on)), "enable_counters")

    def enable_kernel_timing(self, on: bool):
        self._chk(self.lib.spcbpt_enable_kernel_timing(self.h, int(on)), "enable_kernel_timing")

    def reset_kernel_time(self):
        self._chk(self.lib.spcbpt_reset_kernel_time(self.h), "reset_kernel_time")

    def kernel_time(self, name: str):
        ms, n = C.c_double(), C.c_int()
        self._chk(self.lib.spcbpt_kernel_time(self.h, name.encode(), C.byref(ms), C.byref(n)), "kernel_time")
        return ms.value, n.value

    def light_info(self):
        """The context's light list (spcbpt_light_info): dicts type (0 QUAD, 1 ENV, 2 MESH), area, n_triangles, first_subspace, n_patches."""
        out = []
        n = self.environment()["n_lights"]
        for k in range(n):
            t, a, nt, fs, npch = C.c_int32(), C.c_float(), C.c_int32(), C.c_int32(), C.c_int32()
            self._chk(self.lib.spcbpt_light_info(self.h, k, C.byref(t), C.byref(a), C.byref(nt), C.byref(fs), C.byref(npch)), "light_info")
            out.append(dict(type=t.value, area=a.value, n_triangles=nt.value, first_subspace=fs.value, n_patches=npch.value))
        return out

    def scene_info(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.lib.spcbpt_scene_info(self.h, C.byref(a), C.byref(b), C.byref(c)), "scene_info")
        return dict(n_triangles=a.value, n_bvh_nodes=b.value, bvh_depth=c.value)

    def trace_closest(self, rays: np.ndarray):
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = r.shape[0]
        t = np.zeros(n, dtype=np.float32)
        tri = np.zeros(n, dtype=np.int32)
        uv = np.zeros((n, 2), dtype=np.float32)
        self._chk(self.lib.spcbpt_trace_closest(self.h, r.ctypes.data, n, t.ctypes.data, tri.ctypes.data, uv.ctypes.data),
                  "trace_closest")
        return t, tri, uv

    def trace_any(self, rays: np.ndarray):
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = r.shape[0]
        vis = np.zeros(n, dtype=np.int32)
        self._chk(self.lib.spcbpt_trace_any(self.h, r.ctypes.data, n, vis.ctypes.data), "trace_any")
        return vis

    def trace_bench(self, rays: np.ndarray, mode: int, any_hit: bool, repeat: int = 5, stats: bool = True):
        """spcbpt_debug_trace_bench: the same rays through the lane-per-ray (mode 0) or quad-per-ray (mode 1) pool-fed kernels.
        Returns (outputs, avg_ms, stats dict or None); outputs = visibility, or (t, tri, uv)."""
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = r.shape[0]
        ms = C.c_double(0.0)
        st = (C.c_uint64 * 5)()
        if any_hit:
            vis = np.zeros(n, dtype=np.int32)
            self._chk(self.lib.spcbpt_debug_trace_bench(self.h, r.ctypes.data, n, int(mode), 1, int(repeat), None, None, None, vis.ctypes.data,
                                                        C.byref(ms), st if stats else None), "debug_trace_bench")
            out = vis
        else:
            t = np.zeros(n, dtype=np.float32); tri = np.zeros(n, dtype=np.int32); uv = np.zeros((n, 2), dtype=np.float32)
            self._chk(self.lib.spcbpt_debug_trace_bench(self.h, r.ctypes.data, n, int(mode), 0, int(repeat), t.ctypes.data, tri.ctypes.data, uv.ctypes.data, None,
                                                        C.byref(ms), st if stats else None), "debug_trace_bench")
            out = (t, tri, uv)
        sd = dict(zip(("node_visits", "leaf_visits", "tri_tests", "lane_slots", "lanes_busy"), [int(x) for x in st])) if stats else None
        return out, float(ms.value), sd

    def trace_pool(self, own_rays: np.ndarray, own_mask: np.ndarray, shadow_org: np.ndarray, shadow_rays: np.ndarray):
        """spcbpt_debug_trace_pool: ONE pooled traversal pass of the eye megakernel over n lanes (lane i = lane i % 64 of wave i // 64).
        own_rays (n, 8) [o, -, d, -] are traced where own_mask (n,) is set, over (SCENE_EPSILON, 1e16); shadow_org (n, 3 or 4) are the lanes'
        eye vertices; shadow_rays (n, CONNECTION_N, 4) hold [direction, length], length < 0 = empty slot, traced over
        (SCENE_EPSILON, length - SCENE_EPSILON).  Returns (t, tri, uv, lengths): the own rays' hits and the (n, CONNECTION_N) slot
        lengths after the pass, -1 where the ray was occluded."""
        own = np.ascontiguousarray(own_rays, dtype=np.float32).reshape(-1, 8)
        n = own.shape[0]
        mask = np.ascontiguousarray(own_mask, dtype=np.int32).reshape(-1)
        org = np.zeros((n, 4), dtype=np.float32)
        org[:, :3] = np.asarray(shadow_org, dtype=np.float32).reshape(n, -1)[:, :3]
        sh = np.array(shadow_rays, dtype=np.float32, order="C").reshape(-1, 4)   # a copy: the call writes the answers into it
        if mask.shape[0] != n or sh.shape[0] != n * CONNECTION_N:
            raise ValueError("trace_pool: own_mask is (n,), shadow_rays (n, CONNECTION_N, 4)")
        t = np.zeros(n, dtype=np.float32); tri = np.zeros(n, dtype=np.int32); uv = np.zeros((n, 2), dtype=np.float32)
        self._chk(self.lib.spcbpt_debug_trace_pool(self.h, n, own.ctypes.data, mask.ctypes.data, org.ctypes.data, sh.ctypes.data, t.ctypes.data,
                                                   tri.ctypes.data, uv.ctypes.data), "debug_trace_pool")
        return t, tri, uv, sh.reshape(n, CONNECTION_N, 4)[:, :, 3].copy()

    # -- the reference's per-frame sequence (optixPathTracer.cpp:791-822) ------
    def render_frame(self, alg: str, subframe: int, launch_frame: Optional[int] = None, rows=None):
        """One frame of `alg`; the algorithms that read a light-vertex cache ("SPCBPT_eye", "SPCBPT_no_rmis", "lt") get their light
        pass (launch frame subframe + 1 unless given) and sampler build first."""
        if alg in ("SPCBPT_eye", "SPCBPT_no_rmis", "lt"):
            self.launch("light trace", subframe + 1 if launch_frame is None else launch_frame)
            self.build_sampler()
        self.launch(alg, subframe, rows)
