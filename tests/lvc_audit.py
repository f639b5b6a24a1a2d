"""Float64 audit of a light-vertex cache, record by record, from the cache's own previous records (a helper, not a test).

A vertex at depth k > 0 is stored directly behind its predecessor (same path_id, depth k - 1: the compact cache is in (core, slot)
order), and every field of it is a closed-form function of the predecessor record (for depth >= 2 also of the record before that),
of the scene's materials and of the subspace tuple.  audit() recomputes every field from those in float64 numpy and returns, per
check, the error of every record and a conditioning number; judge() holds them to the bars below.  No lock-step with the oracle, no
common prefix, nothing that a Russian-roulette flip can shift: every record is judged.  The Disney Eval / Pdf below are written from
csrc/dev_bsdf.h and keep the reference's quirks as they stand: the max(0.001, roughness) clamp; Pdf mixes GTR1 by 1 / (1 + clearcoat)
although Sample never draws the clearcoat lobe; Eval == 0 for N.L <= 0 or N.V <= 0; a material flagged `brdf` divides the flux
multiplier by |n . dir|.  Only integer labels go through the oracle (ob.tree_index, pinned bit-exact by test_tree_labels_exact).

Definitions (l = predecessor, m = the vertex, p = the record before l; d = normalize(m.P - l.P), t = |m.P - l.P|; behind an origin
on the environment map (flag SPCBPT_LV_DIRECTION) d = l.normal and there is no 1 / t^2):
  pdf_G        |m.n . d| |l.n . d| / t^2
  single_pdf   nsp pdf_G / |l.n . d|, nsp = |l.n . d| / pi at depth 1 (project_pdf = 1 / (pi r^2) behind a sky origin), else
               Pdf(mat_l, l.n, -d_prev, d) rr(l.color): roulette survival is folded in; rr = max(max3(color), MIN_RR_RATE)
  pdf          l.pdf m.single_pdf
  flux         l.flux pdf_G at depth 1, else brdf_div(Eval(mat_l, l.n, -d_prev, d)) l.flux pdf_G
  last_lum     sum_rgb l.flux / l.pdf;      last_normal_projection |l.n . d| (judged absolutely: a cosine)
  rmis_pointer l.rmis_pointer / l.single_pdf at depth 1 (exact in FP32), else
               (l.rmis_pointer LL_pdf + Gamma^[e][l.last_zone_id] l.last_lum CONNECTION_N) / l.single_pdf,
               LL_pdf = Pdf(mat_l, l.n, d, normalize(l.last_position - l.P)) / |l.last_position - l.P|^2 l.last_normal_projection rr(l.color)
               (no area measure and no projection where l carries SPCBPT_LV_LAST_DIRECTION), Gamma^[e][z] = (cmf[e][z] - cmf[e][z-1]) / Q[z]
               with the difference in FP32 as the device takes it, e = eye-tree label of (l.P, l.n, d).
Directions are rebuilt from stored FP32 positions, so the check itself is ill-conditioned for a short segment and for a narrow GGX
lobe.  Every formula is therefore evaluated again, in N_PATTERNS fixed sign patterns, with
  * the three positions moved by +-1 FP32 ulp per coordinate.  The ulp is taken at no less than a quarter of the scene's extent (a hit
    point is a barycentric sum of corners of the scene's size: its rounding does not shrink where a coordinate passes zero) and is
    divided by the cosine of the ray that ARRIVED at the vertex, up to 1e4 (the barycentrics are quotients by a determinant
    proportional to that cosine; an origin is sampled, not traced: one ulp);
  * the two directions handed to Eval / Pdf made one FP32 ulp longer / shorter: where the walk runs nearly straight through a surface
    (L ~ -V: a specular sample below the hemisphere) L . H = (|L|^2 + L . V) / |L + V| is a difference of the directions' LENGTHS,
    and FP32 unit vectors are of unit length to an ulp only.
The largest change is the record's kappa and a record is held to bar + C_KAPPA kappa.  Where C_KAPPA kappa exceeds ILL_KAPPA the
record is ill-conditioned: it is held to the flat LOOSE_BAR instead -- or, where its own slack C_KAPPA kappa exceeds even LOOSE_BAR, to
that slack alone (near L ~ -V one ulp of a direction's length moves L . H by 2 ulp / |L + V|^2; over 48 oracle caches the 85 records of
that band reach 0.33 of their slack, two of them 0.054 and 0.12) -- and at most ILL_CAP of a scenario's records may be ill-conditioned:
beyond that the audit fails and says so, it does not quietly judge fewer records.  Where an ulp moves the value by POLE_KAPPA of itself
the formula has a pole within rounding and nothing bounds the FP32 value (the oracle's own cache holds such records off by 0.25, 0.5
and 4.8): counted among the ill-conditioned, printed, not judged.

Bars (judge): see BARS; how they were derived from the oracle's own cache under this audit is written in tests/test_gpu_lvc_audit.py."""
from __future__ import annotations

import numpy as np

from tests import env_ref

NUM_SUBSPACE = 1000
CONNECTION_N = 3
MIN_RR_RATE = 0.3
SCENE_EPSILON = 1e-3
LV_DIRECTION = 0x80000000
LV_LAST_DIRECTION = 0x40000000
MAX_DEPTH = 52
N_PATTERNS = 6
EPS32 = 2.0 ** -23
FLOAT_FIELDS = ("position", "pdf", "normal", "single_pdf", "flux", "rmis_pointer", "color", "last_lum", "last_position", "last_normal_projection")

# MaterialData() defaults (tests/test_gpu_units.py::_bsdf_records, api.Scene.desc)
MAT_DEFAULTS = dict(metallic=0.0, roughness=0.5, specular=0.5, specular_tint=0.0, subsurface=0.0, sheen=0.0, sheen_tint=0.5, clearcoat=0.0,
                    clearcoat_gloss=1.0, brdf=0, albedo_tex=0)

# ---- bars ---------------------------------------------------------------------------------------------------------------------
# Every bar is a margin over what the ORACLE's cache measures under this audit, never over what the device measures: the four CPU
# scenarios of tests/test_lvc_audit_cpu.py at six launch frames each (1, 2, 3, 7, 11, 12: 24 caches, 220 000 records; the test holds
# the oracle to these bars on frame 7 and prints its figures; tests/test_gpu_lvc_audit.py lists them next to the device's).
#   C_KAPPA     2: the largest power of two at which the oracle stays inside ILL_CAP on every one of the 24 caches (ill-conditioned
#               share of a cache at most 0.29 % / 0.34 % / 0.54 % / 0.78 % for c = 1 / 2 / 4 / 8: the bedroom's 0.05-roughness metal);
#               a smaller c explains less of the conditioning and only widens the bars below.
#   99.9 % bar  4 x the oracle's largest 99.9 % quantile of max(err - c kappa, 0) over the well-conditioned records, floored at 2e-6;
#   hard bar    4 x the oracle's largest maximum of it, and no less than the 99.9 % bar.
C_KAPPA = 2.0
ILL_KAPPA = 1e-2      # a record whose C_KAPPA kappa exceeds this is held to the flat LOOSE_BAR instead (to its slack alone where that is larger) ...
LOOSE_BAR = 5e-2
POLE_KAPPA = 0.5      # ... unless an ulp moves the value by half of itself: the formula has a pole within rounding (L ~ -V: 1 / |L . H|), no bound holds
ILL_CAP = 5e-3        # ... and there may be at most this share of them in a scenario's cache
LABEL_CAP = 1e-3      # labels within rounding of a split / a patch border; sky origins within SKY_BORDER of a texel border
SKY_BORDER = 1e-4     # texels (BORDER of tests/test_gpu_env_first_principles.py)
SKY_UV = 1e-6         # |u - u64|, |v - v64| of the FP32 dir2uv: a few ulps of 1 (atan2f, acosf, the scaling)
BARS = {                                   # field: (99.9 % bar, hard bar)   oracle, c = 2: largest 99.9 % quantile / maximum over the 24 caches
    "origin pdf": (2e-6, 2e-6),                    # 0 / 0: the correctly rounded FP32 quotient
    "origin pdf (sky)": (8.4e-4, 1e-3),            # 2.1e-4 / 2.5e-4: env_pdf takes the FP32 difference of two table entries (test_env_pdf_and_label holds it to 1e-3 too)
    "pdf": (2e-6, 2e-6),                           # 0 / 0: one correctly rounded FP32 product
    "last_lum": (2e-6, 2e-6),                      # 1.5e-7 / 1.7e-7
    "last_normal_projection": (2e-6, 3.4e-6),      # 2.3e-7 / 8.4e-7
    "single_pdf depth 1": (2e-6, 1.4e-5),          # 2.2e-7 / 3.5e-6
    "flux depth 1": (2e-6, 1.4e-5),                # 1.9e-7 / 3.5e-6
    "single_pdf": (1.24e-4, 7.6e-4),               # 3.1e-5 / 1.9e-4
    "flux": (1.24e-4, 7.6e-4),                     # 3.1e-5 / 1.9e-4
    "rmis_pointer": (1.84e-4, 8e-4),               # 4.6e-5 / 2.0e-4
}


# ---- Disney BSDF in float64 (csrc/dev_bsdf.h) -----------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(-1)


def _unit(v):
    return v / np.sqrt(_dot(v, v))[..., None]


def _lerp(a, b, t):
    return a + t * (b - a)


def _schlick(u):
    m = np.clip(1.0 - u, 0.0, 1.0)
    return m * m * m * m * m


def _gtr1(ndh, a):
    a2 = a * a
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (a2 - 1.0) / (np.pi * np.log(a2) * (1.0 + (a2 - 1.0) * ndh * ndh))
    return np.where(a >= 1.0, 1.0 / np.pi, v)


def _gtr2(ndh, a):
    a2 = a * a
    t = 1.0 + (a2 - 1.0) * ndh * ndh
    return a2 / (np.pi * t * t)


def _smith(ndv, alpha_g):
    a, b = alpha_g * alpha_g, ndv * ndv
    return 1.0 / (ndv + np.sqrt(a + b - a * b))


def materials_of(scene, material_id, color):
    """Per-record material arrays: scene.materials[material_id] with the MaterialData() defaults, every parameter rounded to FP32 as
    the C ABI stores it, the base colour replaced by the record's own `color` (load_pbr_colored)."""
    mid = np.asarray(material_id, np.int64)
    out = {}
    for k, dflt in MAT_DEFAULTS.items():
        table = np.array([np.float32(m.get(k, dflt)) for m in scene.materials], np.float64)
        out[k] = table[np.clip(mid, 0, len(table) - 1)]
    out["base"] = np.asarray(color, np.float64)
    return out


def disney_eval(M, N, V, L):
    with np.errstate(divide="ignore", invalid="ignore"):
        ndl, ndv = _dot(N, L), _dot(N, V)
        H = _unit(L + V)
        ndh, ldh = _dot(N, H), _dot(L, H)
        cd = M["base"]
        lum = 0.3 * cd[..., 0] + 0.6 * cd[..., 1] + 0.1 * cd[..., 2]
        ctint = np.where((lum > 0)[..., None], cd / np.where(lum > 0, lum, 1.0)[..., None], 1.0)
        met, rough = M["metallic"], M["roughness"]
        cspec0 = _lerp((M["specular"] * 0.08)[..., None] * _lerp(1.0, ctint, M["specular_tint"][..., None]), cd, met[..., None])
        fl, fv = _schlick(ndl), _schlick(ndv)
        fd90 = 0.5 + 2.0 * ldh * ldh * rough
        fd = _lerp(1.0, fd90, fl) * _lerp(1.0, fd90, fv)
        fss90 = ldh * ldh * rough
        fss = _lerp(1.0, fss90, fl) * _lerp(1.0, fss90, fv)
        ss = 1.25 * (fss * (1.0 / (ndl + ndv) - 0.5) + 0.5)
        ds = _gtr2(ndh, np.maximum(0.001, rough))
        fh = _schlick(ldh)
        fs = _lerp(cspec0, 1.0, fh[..., None])
        rg = (rough * 0.5 + 0.5) ** 2
        gs = _smith(ndl, rg) * _smith(ndv, rg)
        csheen = _lerp(1.0, ctint, M["sheen_tint"][..., None])
        diffuse = (_lerp(fd, ss, M["subsurface"]) / np.pi)[..., None] * cd + (fh * M["sheen"])[..., None] * csheen
        out = diffuse * (1.0 - met)[..., None] + (gs * ds)[..., None] * fs
        dr = _gtr1(ndh, _lerp(0.1, 0.001, M["clearcoat_gloss"]))
        gr = _smith(ndl, 0.25) * _smith(ndv, 0.25)
        out = out + (0.25 * M["clearcoat"] * gr * _lerp(0.04, 1.0, fh) * dr)[..., None]
        return np.where(((ndl <= 0) | (ndv <= 0))[..., None], 0.0, out)


def disney_pdf(M, N, V, L):
    with np.errstate(divide="ignore", invalid="ignore"):
        alpha = np.maximum(0.001, M["roughness"])
        dr = 0.5 * (1.0 - M["metallic"])
        H = _unit(L + V)
        c = np.abs(_dot(H, N))
        g2 = _gtr2(c, alpha) * c
        g1 = _gtr1(c, _lerp(0.1, 0.001, M["clearcoat_gloss"])) * c
        spec = _lerp(g1, g2, 1.0 / (1.0 + M["clearcoat"])) / (4.0 * np.abs(_dot(L, H)))
        return dr * np.abs(_dot(L, N)) / np.pi + (1.0 - dr) * spec


def rr_of(color):
    return np.maximum(np.asarray(color, np.float64).max(-1), MIN_RR_RATE)


def gamma_hat(q, cmf):
    """Gamma^[e][z] = (cmf[e][z] - cmf[e][z - 1]) / Q[z]: the difference in FP32 (gamma_ss), then widened."""
    cmf = np.asarray(cmf, np.float32).reshape(NUM_SUBSPACE, NUM_SUBSPACE)
    g = cmf.copy()
    g[:, 1:] = cmf[:, 1:] - cmf[:, :-1]
    return g.astype(np.float64) / np.asarray(q, np.float32).astype(np.float64)[None, :]


# ---- the scene as the library assembles it --------------------------------------------------------------------------------------
def scene_lights(scene, env):
    """The light list in the library's order (quads, mesh lights, the environment map last) with each light's first patch."""
    from __graft_entry__ import load_package
    api = load_package().api
    V = np.asarray(scene.vertices, np.float32)
    lights, base = [], 0
    for q in scene.lights:
        p, u, v = (np.asarray(q[k], np.float32).astype(np.float64) for k in ("position", "u", "v"))
        cr = np.cross(u, v)
        lights.append(dict(type=0, corner=p, u=u, v=v, normal=cr / np.linalg.norm(cr), area=float(np.linalg.norm(cr)),
                           emission=np.asarray(q["emission"], np.float32), div=int(q.get("div_level", 1)), base=base))
        base += int(q.get("div_level", 1)) ** 2
    for ml in getattr(scene, "mesh_lights", []) or []:
        F = np.asarray(scene.indices)[np.asarray(scene.tri_material) == ml["material"]]
        t = api.mesh_light_table(V, F, ml.get("n_patches", 4))
        lights.append(dict(type=2, tris=V[F[t["tri"]]].astype(np.float64), patch=t["patch"], area=float(np.float32(t["area"])),
                           emission=np.asarray(ml["emission"], np.float32), div=int(t["n_patches"]), base=base))
        base += int(t["n_patches"])
    if env is not None:
        for L in lights:
            L["base"] += 100      # scene_shift.cpp:110: with a sky the patches start at NUM_SUBSPACE_LIGHTSOURCE / 2
        lights.append(dict(type=1, raster=np.asarray(env["rgba"], np.float32), center=np.asarray(env["center"], np.float32).astype(np.float64),
                           r=float(np.float32(env["radius"])), div=10))
    return lights


def scene_triangles(scene, lights):
    """(corners (T, 3, 3) float64, material (T,), emitter (T,) bool): the scene's triangles, then two per quad light (capi.hip:
    corner, corner + u, corner + u + v / corner, corner + u + v, corner + v).  Triangles of a mesh light are emitters in place."""
    P = np.asarray(scene.vertices, np.float32)[np.asarray(scene.indices)].astype(np.float64)
    mat = np.asarray(scene.tri_material, np.int64).copy()
    emit = np.zeros(len(P), bool)
    for ml in getattr(scene, "mesh_lights", []) or []:
        emit |= mat == ml["material"]
    mat[emit] = -1                                 # no surface vertex can carry an emitter's pseudo-material
    quads = []
    for L in lights:
        if L["type"] == 0:
            c, a, b = L["corner"], L["corner"] + L["u"], L["corner"] + L["v"]
            a, b = a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
            p3 = (a + b - c).astype(np.float32).astype(np.float64)
            quads += [np.stack([c, a, p3]), np.stack([c, p3, b])]
    if quads:
        P = np.concatenate([P, np.stack(quads)])
        mat = np.concatenate([mat, np.full(len(quads), -1)])
        emit = np.concatenate([emit, np.ones(len(quads), bool)])
    return P, mat, emit


# ---- results ----------------------------------------------------------------------------------------------------------------------
class Check:
    """One check: `idx` the records judged, `err` their error; `kappa` their conditioning number (None: an exact check or a geometric
    one with a tolerance of its own, where err > 0 is a violation); `cap`: the share of violations tolerated (labels at a split)."""

    def __init__(self, name, idx, err, kappa=None, cap=0.0):
        self.name, self.idx, self.err = name, np.asarray(idx, np.int64), np.asarray(err, np.float64)
        self.kappa = None if kappa is None else np.asarray(kappa, np.float64)
        self.cap = cap


def _rel(a, b):
    """|a - b| over the magnitude of b (vectors: the largest component of the difference over the largest component); NaN = inf"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore"):
        if a.ndim > 1:
            e = np.abs(a - b).max(-1) / (np.abs(b).max(-1) + 1e-300)
        else:
            e = np.abs(a - b) / (np.abs(b) + 1e-300)
    with np.errstate(over="ignore"):
        b32 = b.astype(np.float32).astype(np.float64)                # equal zeros; a pdf that overflows FP32 on a long path is stored as inf
    same = ((a == b) | (a == b32)).all(-1) if a.ndim > 1 else (a == b) | (a == b32)
    e = np.where(same, 0.0, e)
    return np.where(np.isnan(e), np.inf, e)


def _f64(x):
    return np.asarray(x, np.float64)


def _predict(S, dPp, dPl, dPm, len_d=1.0, len_p=1.0):
    """Every formula of the module docstring for the step records S (arrays of l, m, p fields), with the three positions displaced
    and the two directions handed to Eval / Pdf scaled by len_d / len_p (an FP32 unit vector is of unit length to an ulp only)."""
    Pm, Pl, Pp = S["mP"] + dPm, S["lP"] + dPl, S["pP"] + dPp
    seg = Pm - Pl
    t2 = _dot(seg, seg)
    d = np.where(S["l_sky"][:, None], S["lN"], seg / np.sqrt(t2)[:, None])
    with np.errstate(divide="ignore", invalid="ignore"):
        dprev = np.where(S["p_sky"][:, None], S["pN"], _unit(Pl - Pp))
    cos_l, cos_m = np.abs(_dot(S["lN"], d)), np.abs(_dot(S["mN"], d))
    pdf_g = np.where(S["l_sky"], cos_m * cos_l, cos_m * cos_l / t2)
    deep = S["deep"]
    with np.errstate(divide="ignore", invalid="ignore"):
        pdf_l = disney_pdf(S["mat"], S["lN"], -dprev * len_p, d * len_d)
        ev = disney_eval(S["mat"], S["lN"], -dprev * len_p, d * len_d)
        next_flux = np.where((S["mat"]["brdf"] != 0)[:, None], ev / cos_l[:, None], ev)
        rr = rr_of(S["l"]["color"])
        nsp = np.where(deep, pdf_l * rr, np.where(S["l_sky"], S["project_pdf"], cos_l / np.pi))
        single_pdf = nsp * pdf_g / cos_l
        lflux = _f64(S["l"]["flux"])
        flux = np.where(deep[:, None], next_flux * lflux * pdf_g[:, None], lflux * pdf_g[:, None])
        # tracing_update_light: the step back from l towards p
        back = Pp - Pl
        out_dir = np.where(S["p_sky"][:, None], -S["pN"], _unit(back))
        pb = disney_pdf(S["mat"], S["lN"], S["ll_sign"][:, None] * d * len_d, out_dir * len_p)
        ll_pdf = np.where(S["l_lld"], pb, pb / _dot(back, back) * _f64(S["l"]["last_normal_projection"])) * rr
        rmis = (_f64(S["l"]["rmis_pointer"]) * ll_pdf + S["gamma"] * _f64(S["l"]["last_lum"]) * CONNECTION_N) / _f64(S["l"]["single_pdf"])
    return dict(single_pdf=single_pdf, flux=flux, lnp=cos_l, rmis=rmis, next_flux=next_flux, pdf_g=pdf_g, d=d, t=np.sqrt(t2), cos_m=cos_m)


def _ulp(P, extent):
    return np.spacing(np.maximum(np.abs(P), 0.25 * extent).astype(np.float32)).astype(np.float64)


def _pairs(lo_a, hi_a, lo_b, hi_b, chunk=1024):
    """Index pairs (i, j) whose boxes [lo_a[i], hi_a[i]] and [lo_b[j], hi_b[j]] overlap (the cheap filter before an exact test)."""
    I, J = [], []
    for a in range(0, len(lo_a), chunk):
        ov = np.ones((min(chunk, len(lo_a) - a), len(lo_b)), bool)
        for k in range(3):
            ov &= (lo_a[a:a + chunk, None, k] <= hi_b[None, :, k]) & (hi_a[a:a + chunk, None, k] >= lo_b[None, :, k])
        i, j = np.nonzero(ov)
        I.append(i + a); J.append(j)
    return np.concatenate(I), np.concatenate(J)


def _locate(points, tris, tol):
    """For every point: over the triangles it lies in (barycentrics >= -1e-4), the least distance to the plane -> (distance, index)."""
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    n = np.cross(e1, e2)
    nn = n / np.linalg.norm(n, axis=1, keepdims=True)
    d11, d12, d22 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
    den = d11 * d22 - d12 * d12
    dist, which = np.full(len(points), np.inf), np.full(len(points), -1, np.int64)
    pad = 64.0 * tol
    i, j = _pairs(points - pad, points + pad, tris.min(1), tris.max(1))
    w = points[i] - tris[j, 0]
    h = np.abs(_dot(w, nn[j]))
    w1, w2 = _dot(w, e1[j]), _dot(w, e2[j])
    u, v = (d22[j] * w1 - d12[j] * w2) / den[j], (d11[j] * w2 - d12[j] * w1) / den[j]
    h = np.where((u >= -1e-4) & (v >= -1e-4) & (u + v <= 1 + 1e-4), h, np.inf)
    order = np.lexsort((h, i))                                       # per point, the nearest plane first
    firsts = order[np.concatenate([[True], i[order][1:] != i[order][:-1]])] if len(order) else order
    dist[i[firsts]], which[i[firsts]] = h[firsts], j[firsts]
    return dist, which, nn


def _crossings(A, B, tris, emit, tri_n, tol):
    """Number of triangles the open segment A -> B crosses (Moller-Trumbore in float64): ray parameter in [kEps / t, 1 - 1e-4], both
    barycentrics and their complement above 1e-4; an emitter seen from behind does not count (path rays pass through it), nor does a
    triangle in whose plane B lies to `tol` (on a segment of a few millimetres the stored hit point's rounding exceeds 1e-4 of t)."""
    hits = np.zeros(len(A), np.int64)
    i, j = _pairs(np.minimum(A, B), np.maximum(A, B), tris.min(1), tris.max(1))
    e1, e2 = (tris[:, 1] - tris[:, 0])[j], (tris[:, 2] - tris[:, 0])[j]
    o, D = A[i], (B - A)[i]
    t = np.sqrt(_dot(D, D))
    with np.errstate(divide="ignore", invalid="ignore"):
        pv = np.cross(D, e2)
        det = _dot(pv, e1)
        tv = o - tris[j, 0]
        u = _dot(tv, pv) / det
        qv = np.cross(tv, e1)
        v = _dot(qv, D) / det
        s = _dot(qv, e2) / det
        back = emit[j] & (_dot(D, tri_n[j]) > 0)
        nu = tri_n[j] / np.sqrt(_dot(tri_n[j], tri_n[j]))[:, None]
        own = np.abs(_dot(B[i] - tris[j, 0], nu)) <= tol              # B lies in this triangle's plane: the surface it hit, not one it crossed
        hit = ~own & (np.abs(det) > 0) & (u > 1e-4) & (v > 1e-4) & (u + v < 1 - 1e-4) & (s >= SCENE_EPSILON / t) & (s <= 1 - 1e-4) & ~back
    np.add.at(hits, i[hit], 1)
    return hits


# ---- the audit ---------------------------------------------------------------------------------------------------------------------
def audit(scene, tuple_, lvc, light_trace_geometry, env=None, path_count=None):
    """scene: api.Scene; tuple_: (eye_tree, light_tree, q, cmf_gamma) as get_subspace() returns it; lvc: the compact cache;
    light_trace_geometry: (num_core, core_padding, m_per_core); env: scene.environment of a scene with a sky; path_count: the
    sampler's path count (sampler_read()[4]) if it is to be checked.  Returns {name: Check}."""
    from oracle import binding as ob
    eye_tree, light_tree, q, cmf = tuple_
    num_core, core_padding, m_per_core = (int(x) for x in light_trace_geometry)
    n = len(lvc)
    out = {}
    idx_all = np.arange(n)
    depth = lvc["depth"].astype(np.int64)
    pid = lvc["path_id"].astype(np.int64)
    flags = lvc["pad"] & np.uint32(LV_DIRECTION | LV_LAST_DIRECTION)
    lights = scene_lights(scene, env)
    n_lights = len(lights)
    tris, tri_mat, tri_emit = scene_triangles(scene, lights)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    extent = float(np.linalg.norm(hi - lo))
    pos_tol = 4.0 * float(np.spacing(np.float32(extent)))

    # ---- structure
    prev_ok = np.zeros(n, bool)
    prev_ok[1:] = (pid[1:] == pid[:-1]) & (depth[1:] == depth[:-1] + 1)
    step = depth > 0
    out["structure: predecessor"] = Check("structure: predecessor", idx_all[step], (~prev_ok[step]).astype(float))
    out["structure: depth"] = Check("structure: depth", idx_all, ((depth < 0) | (depth > MAX_DEPTH)).astype(float))
    org = np.nonzero(depth == 0)[0]
    core, k = pid[org] // m_per_core, pid[org] % m_per_core
    first = np.ones(len(org), bool)
    first[1:] = core[1:] != core[:-1]
    want_k = np.where(first, 0, np.concatenate([[0], k[:-1] + 1]))
    bad = (k != want_k) | (core < 0) | (core >= num_core)
    bad[1:] |= core[1:] < core[:-1]
    out["structure: path ids"] = Check("structure: path ids", org, bad.astype(float))
    rec_core = np.clip(pid // m_per_core, 0, num_core - 1)
    per_core = np.bincount(rec_core, minlength=num_core)
    paths_core = np.bincount(np.clip(core, 0, num_core - 1), minlength=num_core)
    # every core starts a path, fills at most its slot range, and stops short of m_per_core paths only because the range is full
    cbad = (per_core > core_padding) | (paths_core < 1) | ((paths_core < m_per_core) & (per_core != core_padding))
    out["structure: cores"] = Check("structure: cores", np.arange(num_core), cbad.astype(float))
    if path_count is not None:
        out["structure: path count"] = Check("structure: path count", [0], [float(len(org) != int(path_count))])

    # ---- flags: DIRECTION on sky origins, LAST_DIRECTION on their successors, nowhere else
    sky_org = np.zeros(n, bool)
    if env is not None:
        sky_org[org] = lvc["material_id"][org] == n_lights - 1
    want_flags = np.where(sky_org, np.uint32(LV_DIRECTION), np.uint32(0))
    succ = np.zeros(n, bool)
    succ[1:] = sky_org[:-1] & step[1:]
    want_flags = want_flags | np.where(succ, np.uint32(LV_LAST_DIRECTION), np.uint32(0))
    out["flags"] = Check("flags", idx_all, (flags != want_flags).astype(float))

    # ---- origin vertices
    P, N = _f64(lvc["position"]), _f64(lvc["normal"])
    o_err = {k_: np.zeros(len(org)) for k_ in ("position", "normal", "pdf", "exact", "label", "border", "sky flux")}
    lid = lvc["material_id"][org].astype(np.int64)
    o_err["exact"] += ((lid < 0) | (lid >= n_lights)).astype(float)
    for j, L in enumerate(lights):
        s = np.nonzero(lid == j)[0]
        if not len(s):
            continue
        r = lvc[org[s]]
        p, nr = P[org[s]], N[org[s]]
        if L["type"] == 1:
            dsky = -nr                                                    # the sky direction; the walk runs along d = normal
            o_err["normal"][s] = np.maximum(np.abs(np.sqrt(_dot(nr, nr)) - 1.0) - 1e-6, 0.0)
            rel = p - (L["center"] + 10.0 * L["r"] * dsky)
            tol = 8.0 * float(np.spacing(np.float32(10.0 * L["r"])))
            o_err["position"][s] = np.maximum(np.maximum(np.abs(_dot(rel, dsky)) - tol, np.sqrt(_dot(rel, rel)) - L["r"] - tol), 0.0)
            pdf, edge = env_ref.env_pdf(L["raster"], dsky)
            h, w = L["raster"].shape[:2]
            near = edge < SKY_BORDER                                      # within 1e-4 texel of a border FP32 (u, v) may read the other texel: counted, capped
            o_err["border"][s] = near
            o_err["pdf"][s] = np.where(near, 0.0, np.maximum(_rel(r["pdf"], pdf / n_lights), _rel(r["single_pdf"], pdf / n_lights)))
            # flux = env_color(direction): bilinear lookup of the row-flipped raster.  FP32 atan2 / acos leave (u, v) a few ulps of 1 off
            # (SKY_UV), which the cell's slope turns into colour; the weights and the sum add a few ulps of the cell's largest texel
            u64, v64 = env_ref.dir2uv(dsky)
            contrast, big = env_ref.local_contrast(env_ref.texture(L["raster"]), u64, v64)
            e_col = np.abs(_f64(r["flux"]) - env_ref.env_color(L["raster"], dsky)).max(-1)
            o_err["sky flux"][s] = np.maximum(e_col / (SKY_UV * contrast + 2e-6 * big) - 1.0, 0.0)
            lab, _ = env_ref.env_label(dsky, L["div"])
            o_err["label"][s] = r["subspace_id"] != lab
            o_err["exact"][s] += (r["rmis_pointer"] != 1.0)
            continue
        want_pdf = 1.0 / (L["area"] * n_lights)
        o_err["pdf"][s] = np.maximum(_rel(r["pdf"], want_pdf), _rel(r["single_pdf"], want_pdf))
        o_err["exact"][s] += (r["rmis_pointer"] != 1.0) | (r["flux"] != L["emission"][None, :]).any(1)
        if L["type"] == 0:
            w = p - L["corner"]
            uu, uv, vv = _dot(L["u"], L["u"]), _dot(L["u"], L["v"]), _dot(L["v"], L["v"])
            den = uu * vv - uv * uv
            r1 = (vv * _dot(w, L["u"]) - uv * _dot(w, L["v"])) / den
            r2 = (uu * _dot(w, L["v"]) - uv * _dot(w, L["u"])) / den
            off = np.abs(_dot(w, L["normal"]))
            outside = np.maximum(np.maximum(-r1, r1 - 1), np.maximum(-r2, r2 - 1)) * np.sqrt(max(uu, vv))
            o_err["position"][s] = np.maximum(np.maximum(off, outside) - pos_tol, 0.0)
            o_err["normal"][s] = np.maximum(np.abs(nr - L["normal"][None, :]).max(1) - 1e-6, 0.0)
            xb = np.clip(np.floor(r1 * L["div"]), 0, L["div"] - 1).astype(np.int64)
            yb = np.clip(np.floor(r2 * L["div"]), 0, L["div"] - 1).astype(np.int64)
            o_err["label"][s] = r["subspace_id"] != NUM_SUBSPACE - (L["base"] + xb * L["div"] + yb) - 1
        else:
            dist, which, nn = _locate(p, L["tris"], pos_tol)
            o_err["position"][s] = np.maximum(dist - pos_tol, 0.0)
            o_err["normal"][s] = np.maximum(np.abs(nr - nn[which]).max(1) - 1e-6, 0.0)
            o_err["label"][s] = r["subspace_id"] != NUM_SUBSPACE - (L["base"] + L["patch"][which]) - 1
    out["origin: position"] = Check("origin: position", org, o_err["position"])
    out["origin: normal"] = Check("origin: normal", org, o_err["normal"])
    out["origin: flux, rmis_pointer, material_id"] = Check("origin: flux, rmis_pointer, material_id", org, o_err["exact"])
    sky = sky_org[org]
    out["origin pdf"] = Check("origin pdf", org[~sky], o_err["pdf"][~sky], kappa=np.zeros(int((~sky).sum())))
    if env is not None:   # env_pdf takes the FP32 difference of two entries of the sampling table: tests/test_gpu_env_first_principles.py::test_env_pdf_and_label
        out["origin pdf (sky)"] = Check("origin pdf (sky)", org[sky], o_err["pdf"][sky], kappa=np.zeros(int(sky.sum())))
        out["origin pdf (sky): within 1e-4 texel of a border, pdf not judged"] = Check("origin pdf (sky): within 1e-4 texel of a border, pdf not judged", org[sky], o_err["border"][sky], cap=LABEL_CAP)
        out["origin: flux (sky)"] = Check("origin: flux (sky)", org[sky], o_err["sky flux"][sky])
    out["origin: subspace label"] = Check("origin: subspace label", org, o_err["label"], cap=LABEL_CAP)

    # ---- steps: only records whose predecessor rule holds (the others are named by the structure check)
    mi = np.nonzero(step & prev_ok)[0]
    li = mi - 1
    l_ok = np.concatenate([[False], (step & prev_ok)[:-1]])[mi]                 # depth >= 2: the record before l must be l's predecessor as well
    keep = (depth[mi] == 1) | l_ok
    mi, li = mi[keep], li[keep]
    deep = depth[mi] >= 2
    pi = np.where(deep, mi - 2, li)
    m, l, p = lvc[mi], lvc[li], lvc[pi]
    l_sky, p_sky = sky_org[li], sky_org[pi] & deep
    S = dict(mP=P[mi], lP=P[li], pP=P[pi], mN=N[mi], lN=N[li], pN=N[pi], l=l, deep=deep, l_sky=l_sky, p_sky=p_sky,
             l_lld=(l["pad"] & np.uint32(LV_LAST_DIRECTION)) != 0, mat=materials_of(scene, l["material_id"], l["color"]),
             ll_sign=np.ones(len(mi)), project_pdf=1.0 / (np.pi * lights[-1]["r"] ** 2) if env is not None else 0.0)
    zero = np.zeros((len(mi), 3))
    base = _predict(dict(S, gamma=np.zeros(len(mi))), zero, zero, zero)
    # eye-tree label of l seen from m, and Gamma^ / Q of (that label, l.last_zone_id)
    e = ob.tree_index(eye_tree, np.concatenate([l["position"], l["normal"], base["d"].astype(np.float32)], 1))
    gh = gamma_hat(q, cmf)
    S["gamma"] = gh[np.clip(e, 0, NUM_SUBSPACE - 1), np.clip(l["last_zone_id"].astype(np.int64), 0, NUM_SUBSPACE - 1)]
    base = _predict(S, zero, zero, zero)

    got = dict(single_pdf=_f64(m["single_pdf"]), flux=_f64(m["flux"]), lnp=_f64(m["last_normal_projection"]), rmis=_f64(m["rmis_pointer"]))

    def err_of(pred):
        return dict(single_pdf=_rel(got["single_pdf"], pred["single_pdf"]), flux=_rel(got["flux"], pred["flux"]),
                    lnp=np.abs(got["lnp"] - pred["lnp"]), rmis=_rel(got["rmis"], pred["rmis"]))

    def spread(a, b):
        a, b = np.asarray(a), np.asarray(b)
        if a.ndim > 1:
            return np.abs(a - b).max(-1) / (np.abs(b).max(-1) + 1e-300)
        return np.abs(a - b) / (np.abs(b) + 1e-300)

    kappa = {k_: np.zeros(len(mi)) for k_ in ("single_pdf", "flux", "lnp", "rmis")}
    rng = np.random.default_rng(0x5EED)
    # a hit point's barycentrics are quotients by the determinant ~ |n . d_in|: its rounding grows as 1 / cosine of the ARRIVING ray
    # (an origin is sampled, not traced: one ulp)
    with np.errstate(divide="ignore", invalid="ignore"):
        cos_in_l = np.where(deep, np.abs(_dot(S["lN"], np.where(p_sky[:, None], S["pN"], _unit(S["lP"] - S["pP"])))), 1.0)
        cos_in_p = np.where(deep & (depth[pi] > 0), np.abs(_dot(S["pN"], _unit(S["pP"] - _f64(p["last_position"])))), 1.0)
        graze = [np.clip(1.0 / np.nan_to_num(c_, nan=1.0), 1.0, 1e4)[:, None] for c_ in (cos_in_p, cos_in_l, base["cos_m"])]
    up, ul, um = _ulp(S["pP"], extent) * graze[0], _ulp(S["lP"], extent) * graze[1], _ulp(S["mP"], extent) * graze[2]
    for k_pat in range(N_PATTERNS):
        sg = rng.choice([-1.0, 1.0], size=(3, 1, 3))               # one fixed sign pattern per evaluation, the same for every record
        ln = (1.0 + EPS32, 1.0 - EPS32) if k_pat % 2 else (1.0 - EPS32, 1.0 + EPS32)
        pr = _predict(S, sg[0] * up, sg[1] * ul, sg[2] * um, *ln)
        with np.errstate(invalid="ignore"):
            for k_ in ("single_pdf", "flux", "rmis"):
                kk = spread(pr[k_], base[k_])
                kappa[k_] = np.maximum(kappa[k_], np.where(np.isnan(kk), np.inf, kk))
            kappa["lnp"] = np.maximum(kappa["lnp"], np.abs(pr["lnp"] - base["lnp"]))
    err = err_of(base)
    d1 = ~deep
    out["single_pdf depth 1"] = Check("single_pdf depth 1", mi[d1], err["single_pdf"][d1], kappa["single_pdf"][d1])
    out["flux depth 1"] = Check("flux depth 1", mi[d1], err["flux"][d1], kappa["flux"][d1])
    out["single_pdf"] = Check("single_pdf", mi[deep], err["single_pdf"][deep], kappa["single_pdf"][deep])
    out["flux"] = Check("flux", mi[deep], err["flux"][deep], kappa["flux"][deep])
    out["rmis_pointer"] = Check("rmis_pointer", mi[deep], err["rmis"][deep], kappa["rmis"][deep])
    out["last_normal_projection"] = Check("last_normal_projection", mi, err["lnp"], kappa["lnp"])
    zk = np.zeros(len(mi))
    out["pdf"] = Check("pdf", mi, _rel(m["pdf"], _f64(l["pdf"]) * _f64(m["single_pdf"])), zk)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["last_lum"] = Check("last_lum", mi, _rel(m["last_lum"], (_f64(l["flux"]) / _f64(l["pdf"])[:, None]).sum(1)), zk)
        r1 = l["rmis_pointer"] / l["single_pdf"]                          # FP32 / FP32: tracing_init_light, exact
    out["rmis_pointer depth 1"] = Check("rmis_pointer depth 1", mi[d1], (m["rmis_pointer"][d1] != r1[d1]).astype(float))
    lp_want = np.where(l_sky[:, None], (m["position"] - l["normal"]).astype(np.float32), l["position"])
    lp_err = np.abs(_f64(m["last_position"]) - _f64(lp_want)).max(1)
    lp_err = np.where(l_sky, np.maximum(lp_err - 2.0 * _ulp(S["mP"], extent).max(1), 0.0), lp_err)   # m.P - d: one FP32 subtraction
    out["last_position"] = Check("last_position", mi, lp_err)
    out["last_zone_id"] = Check("last_zone_id", mi, (m["last_zone_id"] != l["subspace_id"]).astype(float))
    mid_ = m["material_id"].astype(np.int64)
    tex = np.array([int(mm.get("albedo_tex", 0)) > 0 for mm in scene.materials])
    base_col = np.array([np.asarray(mm.get("color", (1, 1, 1)), np.float32) for mm in scene.materials])
    valid_mat = (mid_ >= 0) & (mid_ < len(scene.materials))
    plain = valid_mat & ~tex[np.clip(mid_, 0, len(tex) - 1)]
    out["color"] = Check("color", mi[plain], (m["color"][plain] != base_col[mid_[plain]]).any(1).astype(float))
    lab = ob.tree_index(light_tree, np.concatenate([m["position"], m["normal"], (-base["d"]).astype(np.float32)], 1))
    out["subspace label"] = Check("subspace label", mi, (m["subspace_id"] != lab).astype(float), cap=LABEL_CAP)

    # ---- geometry of the step: m lies in a triangle of its material whose unit normal, turned against d, is m.normal
    g_err = np.full(len(mi), np.inf)
    n_err = np.full(len(mi), np.inf)
    for mat_id in np.unique(mid_):
        sel = np.nonzero(mid_ == mat_id)[0]
        cand = np.nonzero(tri_mat == mat_id)[0]
        if not len(cand) or mat_id < 0:
            continue
        dist, which, nn = _locate(S["mP"][sel], tris[cand], pos_tol)
        g_err[sel] = np.maximum(dist - pos_tol, 0.0)
        tn = nn[which]
        tn = np.where((_dot(tn, base["d"][sel]) > 0)[:, None], -tn, tn)
        n_err[sel] = np.maximum(np.abs(tn - S["mN"][sel]).max(1) - 1e-6, 0.0)
    n_err = np.maximum(n_err, np.maximum(_dot(S["mN"], base["d"]) - 1e-6, 0.0))
    out["position on a triangle of the material"] = Check("position on a triangle of the material", mi, g_err)
    out["normal"] = Check("normal", mi, n_err)
    tri_n = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    out["segment is clear"] = Check("segment is clear", mi, _crossings(S["lP"], S["mP"], tris, tri_emit, tri_n, pos_tol).astype(float))
    out["_step"] = dict(mi=mi, li=li, pi=pi, deep=deep, base=base, S=S)          # for the corruption tests: the audit's own intermediate values
    return out


class Failure(tuple):
    """(check, message) of a failed check; .records: the indices of the offending records, worst first"""

    def __new__(cls, name, msg, records):
        t = tuple.__new__(cls, (name, msg))
        t.records = np.asarray(records, np.int64)
        return t


def quantiles(x):
    x = np.asarray(x, np.float64)
    return np.quantile(x, [0.5, 0.99, 0.999, 1.0]) if len(x) else np.zeros(4)


def judge(results, lvc, scenario, bars=None, c_kappa=C_KAPPA, report=print):
    """Holds every check of audit() to its bar.  Returns the list of (check, message) of the failures (empty: the cache passes); every message names
    the check, the scenario, the number of offending records and the first few (path_id, depth).  Prints the error quantiles
    50 / 99 / 99.9 / 100 % of every floating-point check, and the number of capped exemptions."""
    bars = BARS if bars is None else bars
    fails = []
    ill_all = np.zeros(len(lvc), bool)

    def name_records(idx):
        return ", ".join(f"({int(lvc['path_id'][i])}, {int(lvc['depth'][i])})" for i in idx[:5])

    for name, c in results.items():
        if name.startswith("_"):
            continue
        n = len(c.err)
        if c.kappa is None:
            bad = np.nonzero(c.err > 0)[0]
            allowed = int(np.floor(c.cap * n))
            report(f"{scenario}: {name}: {n} records, {len(bad)} violations" + (f" (cap {allowed})" if c.cap else ""))
            if len(bad) > allowed:
                what = name_records(c.idx[bad]) if "cores" not in name and "path count" not in name else "cores " + ", ".join(str(int(i)) for i in c.idx[bad][:5])
                fails.append(Failure(name, f"{scenario}: {name}: {len(bad)} of {n} records violate it (allowed {allowed}); first: {what}", c.idx[bad]))
            continue
        bar, hard = bars[name]
        slack = c_kappa * c.kappa
        slack = np.where(slack >= POLE_KAPPA, np.inf, slack)
        ill = ~(slack <= ILL_KAPPA)
        excess = np.maximum(c.err - np.where(ill, 0.0, slack), 0.0)
        q, qx = quantiles(c.err), quantiles(excess[~ill])
        report(f"{scenario}: {name}: {n} records, ill-conditioned {int(ill.sum())} (of them at a pole: {int(np.isinf(slack).sum())}); error quantiles 50/99/99.9/100 % = " + " ".join(f"{x:.3g}" for x in q)
               + "; over c kappa = " + " ".join(f"{x:.3g}" for x in qx))
        if n == 0:
            continue
        ill_all[c.idx[ill]] = True
        pole = np.isinf(slack)
        # ill-conditioned: the flat LOOSE_BAR; where the record's own slack exceeds even that, the slack alone; at a pole nothing
        over_hard = np.where(ill, ~pole & ~(c.err <= np.maximum(LOOSE_BAR, np.where(pole, 0.0, slack))), excess > hard)
        over_soft = np.where(ill, over_hard, excess > bar)
        size = np.where(ill, c.err, excess)                          # what a record is named by: how far over its own slack it is

        def worst(mask):
            k = np.nonzero(mask)[0]
            return c.idx[k[np.argsort(-size[k])]]
        if over_hard.any():
            fails.append(Failure(name, f"{scenario}: {name}: {int(over_hard.sum())} of {n} records beyond the hard bar {hard:g} + {c_kappa:g} kappa "
                                 f"(max({LOOSE_BAR:g}, {c_kappa:g} kappa) where ill-conditioned; largest {size[over_hard].max():.3g}); first: {name_records(worst(over_hard))}", worst(over_soft)))
        elif float(np.quantile(np.where(ill, 0.0, excess), 0.999)) > bar:
            fails.append(Failure(name, f"{scenario}: {name}: {int(over_soft.sum())} of {n} records beyond {bar:g} + {c_kappa:g} kappa: the 99.9 % quantile misses that bar "
                                 f"(quantiles 50/99/99.9/100 % over c kappa = " + " ".join(f"{x:.3g}" for x in qx) + f"); first: {name_records(worst(over_soft))}", worst(over_soft)))
    name = "ill-conditioned share"
    report(f"{scenario}: {name}: {int(ill_all.sum())} of {len(lvc)} records (cap {ILL_CAP:g}) are ill-conditioned in some check: held to max({LOOSE_BAR:g}, c kappa), or at a pole")
    if ill_all.sum() > ILL_CAP * len(lvc):
        fails.append(Failure(name, f"{scenario}: {name}: {int(ill_all.sum())} of {len(lvc)} records have c kappa > {ILL_KAPPA:g} in some check, more than {ILL_CAP:g} of the cache; "
                             f"first: {name_records(np.nonzero(ill_all)[0])}", np.nonzero(ill_all)[0]))
    return fails


def failed_checks(fails):
    """The names of the checks judge() failed."""
    return sorted({name for name, _ in fails})
