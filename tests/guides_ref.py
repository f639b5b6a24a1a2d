"""The float64 definition of the reflected guide planes (Renderer.launch_guides), written from the scene's own arrays (numpy only).

Per pixel the primary ray through the pixel centre (+ an offset in pixels) is followed through mirror-like surfaces -- roughness <=
roughness_max and metallic >= metallic_min -- to the first surface that is not one; every segment's hit comes from a float64 caster
over ALL triangles (tests/ray_verdict.py::scene_triangles: the scene's, then two per quad light, the light's culled from behind), over
(1e-3, 1e16).  Nothing of the product is called.  The chain:
    miss of the primary ray    albedo (1, 1, 1), coverage 0, normal 0, depth 0
    emitter (front)            albedo = throughput, coverage 1, the light's normal unfolded, depth = length + t
    followed surface           throughput *= lerp(Cspec0, 1, (1 - |N.d|)^5), length += t, on from o + t d along d - 2 (N.d) N
    any other surface          albedo = throughput x base colour (texture: bilinear, wrap, pow 2.2), coverage 1, N unfolded, length + t
    miss of a later segment    albedo = throughput, coverage 1, the last mirror's N unfolded through those before it, the length up to it
N is the triangle's normal turned against the ray; unfolding reflects a normal about the chain's mirrors in reverse order.
"""
import numpy as np

from tests.ray_verdict import scene_triangles
from tests.test_gpu_features import _texture64

TMIN = float(np.float32(1e-3))   # SPCBPT_SCENE_EPSILON
TMAX = float(np.float32(1e16))

# how a pixel's chain ended
END_MISS0, END_SURFACE, END_EMITTER, END_MISS = 0, 1, 2, 3


def cast(P, culled, o, d, block=512):
    """Closest hit of rays (o, d) (n, 3) float64 over all triangles P (T, 3, 3): (tri (n,) int, -1 for a miss; t; barycentrics (n, 2)).
    The plane distance t = n.(P0 - o) / n.d, then the barycentrics of p = o + t d as linear forms of p -- u = (p - P0).(e2 x n) / |n|^2,
    v = (p - P0).(n x e1) / |n|^2 -- all in float64, as matrix products over the triangles; a culled triangle is hit from its front
    only (n.d < 0), a zero-area one never."""
    n = len(o)
    tri = np.full(n, -1, np.int64)
    tb = np.full(n, np.inf)
    uvb = np.zeros((n, 2))
    P0, e1, e2 = P[:, 0], P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    nrm = np.cross(e1, e2)
    with np.errstate(divide="ignore", invalid="ignore"):
        n2 = (nrm * nrm).sum(1, keepdims=True)
        au, av = np.cross(e2, nrm) / n2, np.cross(nrm, e1) / n2
    nP0, bu, bv = (nrm * P0).sum(1), -(au * P0).sum(1), -(av * P0).sum(1)
    solid = n2[:, 0] > 0
    for b in range(0, n, block):
        oo, dd = o[b:b + block], d[b:b + block]
        with np.errstate(divide="ignore", invalid="ignore"):
            dn = dd @ nrm.T
            t = (nP0[None] - oo @ nrm.T) / dn
            u = (oo @ au.T + bu[None]) + t * (dd @ au.T)
            v = (oo @ av.T + bv[None]) + t * (dd @ av.T)
            ok = solid[None] & (dn != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > TMIN) & (t < TMAX)
            ok &= ~(culled[None] & (dn > 0))
        t = np.where(ok, t, np.inf)
        k = t.argmin(1)
        r = np.arange(len(k))
        hit = np.isfinite(t[r, k])
        tri[b:b + block] = np.where(hit, k, -1)
        tb[b:b + block] = t[r, k]
        uvb[b:b + block, 0], uvb[b:b + block, 1] = u[r, k], v[r, k]
    return tri, tb, uvb


def _tint(base, metallic, specular, specular_tint, cos):
    lum = 0.3 * base[:, 0] + 0.6 * base[:, 1] + 0.1 * base[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        ctint = np.where(lum[:, None] > 0, base / lum[:, None], 1.0)
    c0 = (specular * 0.08)[:, None] * (1.0 + specular_tint[:, None] * (ctint - 1.0))
    c0 = c0 + metallic[:, None] * (base - c0)
    F = np.clip(1.0 - np.abs(cos), 0.0, 1.0) ** 5
    return c0 + F[:, None] * (1.0 - c0)


def primary_rays(eye, U, V, W, w, h, ox=0.0, oy=0.0):
    y, x = np.mgrid[0:h, 0:w]
    dx = 2.0 * ((x + 0.5 + ox) / w) - 1.0
    dy = 2.0 * ((y + 0.5 + oy) / h) - 1.0
    d = dx[..., None] * U.astype(np.float64) + dy[..., None] * V.astype(np.float64) + W.astype(np.float64)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return d.reshape(-1, 3)


def guide_chain(scene, eye, U, V, W, w, h, max_bounces=4, roughness_max=0.1, metallic_min=0.9, ox=0.0, oy=0.0, geometry=None):
    """-> dict of (h, w, ...) arrays: albedo (.., 4), normal_depth (.., 4) float64, textured bool, end (END_*), bounces (mirrors
    followed), seq (.., max_bounces + 1) int: the triangle of every segment (-1: a miss, -2: no such segment), first (the first
    segment's triangle is a followed mirror)."""
    P, culled, _ = geometry if geometry is not None else scene_triangles(scene)
    roughness_max, metallic_min = float(np.float32(roughness_max)), float(np.float32(metallic_min))   # the parameters are float32
    I = np.asarray(scene.indices, np.int64)
    nt = len(I)
    mat_of = np.asarray(scene.tri_material, np.int64)
    M = scene.materials
    f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)
    color = np.array([f32(m.get("color", (1, 1, 1))) for m in M])
    rough = np.array([float(np.float32(m.get("roughness", 0.5))) for m in M])
    metal = np.array([float(np.float32(m.get("metallic", 0.0))) for m in M])
    spec = np.array([float(np.float32(m.get("specular", 0.5))) for m in M])
    stint = np.array([float(np.float32(m.get("specular_tint", 0.0))) for m in M])
    tex_id = np.array([int(m.get("albedo_tex", 0)) for m in M])
    TC = None if scene.texcoords is None else f32(scene.texcoords)
    n_px = w * h
    d = primary_rays(eye, U, V, W, w, h, ox, oy)
    o = np.tile(np.asarray(eye, np.float32).astype(np.float64), (n_px, 1))
    albedo = np.zeros((n_px, 4)); albedo[:, :3] = 1.0
    nd = np.zeros((n_px, 4))
    textured = np.zeros(n_px, bool)
    end = np.full(n_px, END_MISS0)
    bounces = np.zeros(n_px, np.int64)
    seq = np.full((n_px, max_bounces + 1), -2, np.int64)
    thr = np.ones((n_px, 3))
    length = np.zeros(n_px)
    mirrors = np.zeros((n_px, max(1, max_bounces), 3))   # the normals of the mirrors followed, in order
    live = np.arange(n_px)

    def unfold(idx, n):
        n = n.copy()
        for k in range(max_bounces - 1, -1, -1):
            sel = bounces[idx] > k
            N = mirrors[idx, k]
            n[sel] = (n - 2.0 * (n * N).sum(1, keepdims=True) * N)[sel]
        return n

    for seg in range(max_bounces + 1):
        if len(live) == 0:
            break
        tri, t, uv = cast(P, culled, o[live], d[live])
        seq[live, seg] = tri
        # misses
        ms = tri < 0
        idx = live[ms]
        later = idx[bounces[idx] > 0]
        if len(later):
            k = bounces[later] - 1
            last = mirrors[later, k].copy()
            saved = bounces[later].copy()
            bounces[later] -= 1                       # that mirror's own normal goes through the mirrors BEFORE it
            nn = unfold(later, last)
            bounces[later] = saved
            albedo[later, :3], albedo[later, 3] = thr[later], 1.0
            nd[later, :3], nd[later, 3] = nn, length[later]
            end[later] = END_MISS
        # emitters (front only: the caster culls their backs)
        em = tri >= nt
        idx = live[em]
        if len(idx):
            ln = np.empty((len(idx), 3))
            for j, tr in enumerate(tri[em]):
                L = scene.lights[(tr - nt) // 2]
                c = np.cross(f32(L["u"]), f32(L["v"]))
                ln[j] = c / np.linalg.norm(c)
            albedo[idx, :3], albedo[idx, 3] = thr[idx], 1.0
            nd[idx, :3], nd[idx, 3] = unfold(idx, ln), length[idx] + t[em]
            end[idx] = END_EMITTER
        # surfaces
        sf = (tri >= 0) & (tri < nt)
        idx = live[sf]
        ts, tt, uu = tri[sf], t[sf], uv[sf]
        c = P[ts]
        N = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
        N /= np.linalg.norm(N, axis=1, keepdims=True)
        dd = d[idx]
        N[(N * dd).sum(1) > 0] *= -1.0
        m = mat_of[ts]
        base = color[m].copy()
        tx = tex_id[m] > 0
        for k in np.unique(tex_id[m][tx]):
            s = np.nonzero(tex_id[m] == k)[0]
            T = TC[I[ts[s]]]
            st = (1 - uu[s, 0] - uu[s, 1])[:, None] * T[:, 0] + uu[s, 0, None] * T[:, 1] + uu[s, 1, None] * T[:, 2]
            base[s] = _texture64(np.asarray(scene.textures[k - 1]), st[:, 0], st[:, 1])
        follow = (rough[m] <= roughness_max) & (metal[m] >= metallic_min) & (bounces[idx] < max_bounces)
        stop = ~follow
        si = idx[stop]
        albedo[si, :3], albedo[si, 3] = thr[si] * base[stop], 1.0
        nd[si, :3], nd[si, 3] = unfold(si, N[stop]), length[si] + tt[stop]
        textured[si] = tx[stop]
        end[si] = END_SURFACE
        fi = idx[follow]
        Nf, df = N[follow], dd[follow]
        cos = (Nf * df).sum(1)
        thr[fi] *= _tint(base[follow], metal[m][follow], spec[m][follow], stint[m][follow], cos)
        length[fi] += tt[follow]
        mirrors[fi, bounces[fi]] = Nf
        bounces[fi] += 1
        o[fi] = o[fi] + tt[follow, None] * df
        d[fi] = df - 2.0 * cos[:, None] * Nf
        live = fi
    first = np.zeros(n_px, bool)
    s0 = seq[:, 0]
    on = (s0 >= 0) & (s0 < nt)
    m0 = mat_of[np.where(on, s0, 0)]
    first = on & (rough[m0] <= roughness_max) & (metal[m0] >= metallic_min)
    shape = lambda a: a.reshape((h, w) + a.shape[1:])
    return dict(albedo=shape(albedo), normal_depth=shape(nd), textured=shape(textured), end=shape(end), bounces=shape(bounces),
                seq=shape(seq), first=shape(first))


def guide_truth(scene, eye, U, V, W, w, h, **kw):
    """guide_chain through the pixel centres, with `excluded` (h, w): the chains through the centre and through its four offsets of 1e-3
    pixel disagree on the triangle sequence."""
    geometry = scene_triangles(scene)
    c = guide_chain(scene, eye, U, V, W, w, h, geometry=geometry, **kw)
    excluded = np.zeros((h, w), bool)
    for ox, oy in ((1e-3, 0), (-1e-3, 0), (0, 1e-3), (0, -1e-3)):
        o = guide_chain(scene, eye, U, V, W, w, h, geometry=geometry, ox=ox, oy=oy, **kw)
        excluded |= (o["seq"] != c["seq"]).any(-1)
    c["excluded"] = excluded
    return c


def arms(c):
    """pixels per arm: mirror -> surface, mirror -> mirror -> surface, mirror -> emitter (any number of mirrors), mirror -> miss"""
    ok = ~c["excluded"] if "excluded" in c else np.ones(c["end"].shape, bool)
    e, b = c["end"], c["bounces"]
    return dict(mirror_surface=int((ok & (e == END_SURFACE) & (b == 1)).sum()), mirror_mirror_surface=int((ok & (e == END_SURFACE) & (b == 2)).sum()),
                mirror_emitter=int((ok & (e == END_EMITTER) & (b >= 1)).sum()), mirror_miss=int((ok & (e == END_MISS)).sum()))
