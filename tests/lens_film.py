"""The film "lt" must write through a thin lens, recounted in float64 from the cache it read (a helper, not a test): the recount of
tests/test_gpu_splat.py (_host_film) with the lens of tests/lens_ref.py -- vertex i of the cache is seen from a lens point of its own,
drawn from the stream of slot i (spcbpt_lens_sample_host).  `tracer` answers the shadow rays (Renderer.trace_any or the oracle's): the
kernel's own rays, operation for operation in float32, from the vertex towards its lens point."""
import math

import numpy as np

from tests import lens_ref as L

EPS = np.float32(1e-3)   # SPCBPT_SCENE_EPSILON


def frame(pkg, scene, w, h):
    cam = scene.camera
    U, V, W = pkg.camera_frame(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
    return np.array(cam["eye"], np.float32), U, V, W


def shadow_rays(origin32, pos):
    """From each vertex towards its lens point (float32, as the kernel computes them): (kEps, |c| - kEps)."""
    f = np.float32
    bias = (origin32.astype(f) - pos.astype(f)).astype(f)
    r2 = ((bias[:, 0] * bias[:, 0]).astype(f) + (bias[:, 1] * bias[:, 1]).astype(f)).astype(f)
    r2 = (r2 + (bias[:, 2] * bias[:, 2]).astype(f)).astype(f)
    ln = np.sqrt(r2, dtype=f)
    inv = (f(1.0) / ln).astype(f)
    d = (bias * inv[:, None]).astype(f)
    rays = np.zeros((len(pos), 8), f)
    rays[:, 0:3] = pos
    rays[:, 3] = EPS
    rays[:, 4:7] = d
    rays[:, 7] = (ln - EPS).astype(f)
    return rays


def host_film(pkg, ob, tracer, scene, v, path_count, w, h, radius, focus, subframe=0, edge=1e-4, graze=1e-3):
    """-> (film (h, w, 3), excluded (h, w) bool, lit (h, w) bool, survivors, vertices).  `excluded` marks the pixels whose value hangs on
    a float32 decision, as in tests/test_gpu_splat.py: a vertex lands within `edge` pixel of a pixel edge, or sees its lens point at a
    grazing angle below `graze`."""
    eye, U, V, W = frame(pkg, scene, w, h)
    n = len(v)
    pos = np.asarray(v["position"], np.float32).reshape(-1, 3)
    nrm = np.asarray(v["normal"], np.float64).reshape(-1, 3)
    flux = np.asarray(v["flux"], np.float64).reshape(-1, 3)
    u = pkg.api.lens_sample_host(np.arange(n), subframe, False)[:, 2:4]
    ref = L.splat_lens(eye, U, V, W, w, h, pos, u[:, 0], u[:, 1], radius, focus)
    fx, fy, g, we, O = ref["fx"], ref["fy"], ref["g"], ref["weight"], ref["origin"]
    # the lens points in float32 as the device forms them (the host form's origin does not depend on the pixel)
    o32, _ = pkg.api.camera_lens_ray_host(eye, U, V, W, w, h, np.zeros((n, 2), np.int32), np.full((n, 2), 0.5, np.float32), u, radius, focus)
    c = pos.astype(np.float64) - O
    r2 = (c * c).sum(1)
    to_cam = -c / np.sqrt(r2)[:, None]
    cosb = (nrm * to_cam).sum(1)
    excluded = np.zeros((h, w), bool)
    front = g > 0
    with np.errstate(invalid="ignore"):
        near = front & (fx > -edge) & (fx < w + edge) & (fy > -edge) & (fy < h + edge) & (flux.sum(1) > 0)

    def touch(mask, spread):
        for i in np.nonzero(mask)[0]:
            xs = {int(math.floor(fx[i] + s * spread)) for s in (-1, 0, 1)}
            ys = {int(math.floor(fy[i] + s * spread)) for s in (-1, 0, 1)}
            for y in ys:
                for x in xs:
                    if 0 <= x < w and 0 <= y < h:
                        excluded[y, x] = True
    with np.errstate(invalid="ignore"):
        on_edge = near & ((np.abs(fx - np.round(fx)) < edge) | (np.abs(fy - np.round(fy)) < edge))
        touch(on_edge, edge)
        touch(near & (np.abs(cosb) < graze), 0.0)
        inside = front & (fx >= 0) & (fx < w) & (fy >= 0) & (fy < h)
    live = inside & (cosb > 0) & (flux.sum(1) > 0) & ((v["pad"] & 0x80000000) == 0)
    fb = np.ones((n, 3))
    surf = np.nonzero(live & (v["depth"] != 0))[0]
    lb = np.asarray(v["last_position"], np.float64).reshape(-1, 3) - pos.astype(np.float64)
    lb /= np.linalg.norm(lb, axis=1, keepdims=True)
    keys = np.concatenate([v["material_id"][surf, None].astype(np.float64), np.asarray(v["color"], np.float64).reshape(-1, 3)[surf]], 1)
    for key in np.unique(keys, axis=0):
        sel = surf[(keys == key).all(1)]
        mat = dict(scene.materials[int(key[0])])
        assert not mat.get("brdf", 0)
        mat["color"] = tuple(float(x) for x in key[1:])
        f, _ = ob.bsdf_eval_pdf(mat, np.concatenate([nrm[sel], to_cam[sel], lb[sel]], 1))
        fb[sel] = f.astype(np.float64)
    live &= fb.sum(1) > 0
    idx = np.nonzero(live)[0]
    vis = np.asarray(tracer.trace_any(shadow_rays(o32[idx], pos[idx]))) != 0
    idx = idx[vis]
    with np.errstate(all="ignore"):
        contrib = (flux[idx] / np.asarray(v["pdf"], np.float64)[idx, None]) * fb[idx] * (np.abs(cosb[idx]) / r2[idx] * we[idx] / path_count)[:, None]
    ok = np.isfinite(contrib).all(1)
    idx, contrib = idx[ok], contrib[ok]
    film = np.zeros((h, w, 3))
    px, py = np.floor(fx[idx]).astype(int), np.floor(fy[idx]).astype(int)
    np.add.at(film, (py, px), contrib)
    lit = np.zeros((h, w), bool)
    lit[py, px] = True
    return film, excluded, lit, len(idx), n
