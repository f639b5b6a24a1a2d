"""Float64 definition of the eye side of the estimator -- the connection value with its recursive-MIS weight, the eye vertex a
step of the walk builds, the emitter hit and the sky miss -- and the audit that holds records to it (a helper, not a test).

Written from csrc/dev_rmis.h and csrc/eye_walk.h, quirks as they stand; the Disney Eval / Pdf are tests/bsdf_ref.py's, the
roulette rate, Gamma^ and the conditioning machinery tests/lvc_audit.py's.  a = eye vertex, b = light vertex, N = CONNECTION_N,
rr(v) = max(max3(v.color), MIN_RR_RATE), G^[e][l] = (cmf[e][l] - cmf[e][l - 1]) / Q[l] with the difference and the quotient in FP32.

connect(), general_connection (b.depth > 0), c = normalize(a.P - b.P), r^2 = |a.P - b.P|^2, LA / LB = the unit vectors towards
a's / b's predecessor:
  value    a.flux b.flux fa fb G / (a.pdf b.pdf) w,  G = |a.n . c| |b.n . c| / r^2, fa = div(Eval(a; -c, LA)), fb = div(Eval(b; c, LB));
           div: a material flagged `brdf` divides by |n . c| (not in the cached_plain form, whose scenes have none).
           A component above 1e5 or a NaN turns the whole value into 0 (ISINVALIDVALUE).
  w        W / (W + D_A + D_B),  W = sum_rgb G^[a.sub][b.sub] (b.flux / b.pdf) N
           D_A = sum_rgb (a.R3 LL_A fm_A + wA) pdf_A fm_B (b.flux / b.pdf) / a.single_pdf
           D_B = (b.rmis_pointer LL_B + wB) pdf_B / b.single_pdf
           LL_A = Pdf(a; -c, LA) / |a.lastP - a.P|^2 a.lnp rr(a),  fm_A = div'(Eval(a; -c, LA)) |a.n . LA| / Pdf(a; -c, LA) / rr(a)
           wA = 0 at a.depth == 1, else G^[a.last_zone][light label of a] N
           pdf_A = Pdf(b; LB, c) / r^2 |c . a.n| rr(b),  fm_B = div(Eval(b; LB, c)) |b.n . c| / Pdf(b; LB, c) / rr(b)
           LL_B = Pdf(b; c, LB) / |b.lastP - b.P|^2 b.lnp rr(b)  (no area measure and no projection where b carries
           SPCBPT_LV_LAST_DIRECTION), wB = G^[eye label of b][b.last_zone] b.last_lum N,  pdf_B = Pdf(a; LA, -c) / r^2 |c . b.n| rr(a)
connection_lightSource (b.depth == 0): fb = 0 where b.n . (-c) > 0, else 1 (one-sided);  pdf_A = |b.n . c| / pi |a.n . c| / r^2,
  fm_B = pi,  D_B = b.rmis_pointer pdf_B / b.single_pdf.
The sky direction arm (b carries SPCBPT_LV_DIRECTION, not in cached_plain): c = -b.n; nothing unless a.n . c > 0;
  value = a.flux / a.pdf Eval(a; LA, c) (a.n . c) b.flux / b.pdf w; LL_A takes its incoming direction towards b's POSITION on the sky
  disk, fm_A at -b.n; pdf_A = project_pdf |b.n . a.n|, fm_B = 1 / project_pdf; pdf_B = Pdf(a; LA, -b.n) rr(a) (no area measure);
  D_B = b.rmis_pointer pdf_B / b.single_pdf.
Labels are integers.  form "reference": the light label of a is the light tree's at (a.P, a.n), the eye label of b the eye tree's at
(b.P, b.n), through the oracle's tree_index.  The cached forms use what the record STORES, whatever a tree would say: a's `lsub`
word and the low 16 bits of b.pad minus 1 -- except that a pad label word that is no label (0: an imported cache) on a surface
vertex sends b through the descent.
null pair (the test that skips a connection and its shadow ray): a.n . (-c) <= 0 or b.n . c < 0; sky arm: not a.n . (-b.n) > 0.

eye_vertex(), from the input record (last vertex l, NextVertex.flux / singlePdf, ray direction d) and the hit the device reports
(position, normal, colour, material, t):  pdf_G = |n . d| |l.n . d| / t^2;  flux = l.flux pdf_G (x NextVertex.flux behind the
camera);  single_pdf = NextVertex.singlePdf pdf_G / |l.n . d|;  pdf = l.pdf single_pdf;  last_normal_projection = |l.n . d|;
last_position = l.P;  depth = l.depth + 1;  last_zone_id = l.sub;  rmis3 = 0 at depth 1, else (l.R3 LL_l fm_l + w_l) / l.single_pdf
with in = normalize(P - l.P), w_l = 0 at l.depth == 1 else G^[l.last_zone][light label of l] N.  At the device's own sampled
direction s: NextVertex.flux = div(Eval(n; -d, s)), NextVertex.singlePdf = Pdf(n; -d, s) rr -- the path ends where Pdf is not
positive or the roulette number (the fourth LCG draw of the input seed) exceeds rr.
emitter_hit(): 0 from behind; else l.flux NextVertex.flux Le pdf_G / pdf / R,  R = 1 at depth 1, else 1 + (W + D_A) / pdf_B pdf_L
(rmis::light_hit: the connection_lightSource terms of the virtual light vertex at the hit, D_B = 1).  sky_miss(): the same with the
sky as a direction (no 1 / t^2, no cosine at the sky; pdf_L = env_pdf / n_lights; the flux multiplier towards the sky).

Conditioning: every formula is evaluated again in N_PATTERNS sign patterns with the positions moved by one FP32 ulp (lvc_audit:
the ulp at no less than a quarter of the scene's extent, over the cosine of the arriving ray) and the two directions handed to
Eval / Pdf one ulp longer / shorter, and so the normal; the largest change is the record's kappa and the record is held to bar + C_KAPPA kappa
(lvc_audit.judge: ILL_KAPPA, LOOSE_BAR, POLE_KAPPA, ILL_CAP as there).

Bars (BARS): a margin over what the ORACLE measures under this audit on the CPU (tests/test_connect_definition_cpu.py prints the
figures), never over what the device measures: the 99.9 % bar is 4 x the oracle's largest 99.9 % quantile of max(err - C_KAPPA
kappa, 0) over its families, floored at 2e-6 (the unit bar of tests/test_gpu_units.py for these quantities); the hard bar 4 x its
largest maximum -- and, a deviation from that rule as stated, no less than the 99.9 % bar: a hard bar below the bar that 99.9 % of
the records are held to would be that bar under another name."""
from __future__ import annotations

import numpy as np

from tests import bsdf_ref as B
from tests import env_ref
from tests.lvc_audit import (CONNECTION_N, EPS32, ILL_CAP, LABEL_CAP, LV_DIRECTION, LV_LAST_DIRECTION, N_PATTERNS, NUM_SUBSPACE,  # noqa: F401
                             SCENE_EPSILON, SKY_UV, Check, _ulp, failed_checks, gamma_hat, judge as _judge, rr_of, scene_lights)

FLT_MAX = float(np.finfo(np.float32).max)
INVALID = 100000.0            # ISINVALIDVALUE (raygen.cu:43)
FORMS = ("reference", "cached", "cached_plain")
C_KAPPA = 2.0                 # as lvc_audit: the oracle stays inside ILL_CAP on every family at this factor (figures below)
SIGN_ULP = EPS32              # the null flag is not judged where a cosine lies within one FP32 ulp (of 1) of its sign change

# name: (99.9 % bar, hard bar)   the oracle's largest 99.9 % quantile / maximum of max(err - C_KAPPA kappa, 0) over its families
# (cornell, cornell with a flagged box, courtyard with its sky; eight to ten connection and two eye-step families each, ~3000 records a family:
# tests/test_connect_definition_cpu.py prints them with -s and holds this table to them).  With the conditioning above -- positions,
# the lengths of directions and normals, the lerp of Pdf's two lobes, the connection's cosines -- the oracle leaves nothing
# unexplained beyond two ulps, so every bar sits at the floor; its ill-conditioned share is at most 0.17 % of a family (cap 0.5 %).
BARS = {
    "connect value": (2e-6, 2e-6),                  # 0 / 0
    "connect weight": (2e-6, 2e-6),                 # 9.1e-8 / 1.8e-7
    "eye flux": (2e-6, 2e-6),                       # 0 / 0
    "eye single_pdf": (2e-6, 2e-6),                 # 0 / 0
    "eye pdf": (2e-6, 2e-6),                        # 0 / 0: one correctly rounded FP32 product
    "eye last_normal_projection": (2e-6, 2e-6),     # 1.0e-7 / 1.1e-7 (absolute: a cosine)
    "eye rmis3": (2e-6, 2e-6),                      # 1.4e-7 / 1.7e-7
    "next flux": (2e-6, 2e-6),                      # 2.0e-7 / 2.2e-7
    "next single_pdf": (2e-6, 2e-6),                # 0 / 0
    "emitter radiance": (2e-6, 2e-6),               # 9.6e-8 / 9.7e-8
    # the oracle's light_hit_env weights of escaped camera paths of depth 1 .. 4 (orc_debug_env_partition): 4.0e-6 / 4.7e-6 -- env_pdf is
    # the FP32 difference of two entries of the sampling table.  The oracle returns no sky-miss VALUE: it is the weight times ratios of
    # the inputs times env_color, whose FP32 (u, v) rounding is in the record's kappa (lvc_audit: SKY_UV x the cell's contrast), so
    # the value is held to the weight's bars
    "sky value": (1.6e-5, 1.9e-5),
    "sky weight": (1.6e-5, 1.9e-5),
}


def _f64(x):
    return np.asarray(x, np.float64)


def _dot(a, b):
    return (a * b).sum(-1)


def _unit(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt(_dot(v, v))[..., None]


def _sum3(v):
    return v.sum(-1)


def rel(a, b):
    """|a - b| over the magnitude of b (vectors: the largest component of the difference over the largest component).  Equal zeros
    and NaN on both sides are equal; 1e-30 in the denominator: below FP32's smallest normal number nothing is relative."""
    a, b = _f64(a), _f64(b)
    with np.errstate(invalid="ignore", over="ignore"):
        both_nan = np.isnan(a) & np.isnan(b)
        a, b = np.where(both_nan, 0.0, a), np.where(both_nan, 0.0, b)
        if a.ndim > 1:
            e = np.abs(a - b).max(-1) / (np.abs(b).max(-1) + 1e-30)
            same = ((a == b) | (a == b.astype(np.float32).astype(np.float64))).all(-1)
        else:
            e = np.abs(a - b) / (np.abs(b) + 1e-30)
            same = (a == b) | (a == b.astype(np.float32).astype(np.float64))
    e = np.where(same, 0.0, e)
    return np.where(np.isnan(e), np.inf, e)


def materials(scene, material_id, color):
    """bsdf_ref material of every record: scene.materials[material_id], every parameter rounded to FP32 as the C ABI stores it, the
    base colour replaced by the record's own (load_pbr_colored); "brdf": the flag."""
    mid = np.asarray(material_id, np.int64)
    assert ((mid >= 0) & (mid < len(scene.materials))).all(), "a material id that does not exist"
    M = {k: np.array([np.float32(m.get(k, B.DEFAULTS[k])) for m in scene.materials], np.float64)[mid] for k in B.KEYS}
    M["color"] = _f64(color)
    M["brdf"] = np.array([int(m.get("brdf", 0)) != 0 for m in scene.materials])[mid]
    return M


class _Lens:
    """Eval / Pdf with their two directions and the normal scaled (an FP32 unit vector is of unit length to an ulp only: lvc_audit;
    the normal's length moves N.h, and near the peak of a narrow lobe 1 + (a^2 - 1)(N.h)^2 is a cancellation: bsdf_ref.condition)"""

    def __init__(self, lv=1.0, ll=1.0, ln=1.0, mix=0.0):
        self.lv, self.ll, self.ln, self.mix = lv, ll, ln, mix

    def eval(self, M, N, V, L):
        with np.errstate(all="ignore"):
            return B.eval(M, N * self.ln, V * self.lv, L * self.ll)

    def pdf(self, M, N, V, L):
        """... and Pdf mixes its lobes as g1 + k (g2 - g1), k = 1 / (1 + clearcoat): in FP32 the difference carries an ulp of the
        LARGER lobe even at k = 1, where the clearcoat lobe has no weight -- half a percent of the 0.001-alpha lobe off its peak"""
        with np.errstate(all="ignore"):
            p = B.pdf(M, N * self.ln, V * self.lv, L * self.ll)
            if self.mix:
                _, s2, s1 = B._lobes(M, N * self.ln, V * self.lv, L * self.ll)
                p = p + self.mix * EPS32 * (1.0 - B.diffuse_ratio(M)) * np.maximum(s1, s2)
            return p


def _lens(k):
    """the k-th pattern's lengths"""
    lv, ll = (1.0 + EPS32, 1.0 - EPS32) if k % 2 else (1.0 - EPS32, 1.0 + EPS32)
    return _Lens(lv, ll, 1.0 + EPS32 if k % 4 < 2 else 1.0 - EPS32, mix=1.0 if k % 3 else -1.0)


def _div(M, f, n, d, on):
    """brdf_div"""
    with np.errstate(all="ignore"):
        return np.where((M["brdf"] & on)[..., None], f / np.abs(_dot(n, d))[..., None], f)


def _last_pdf(E, M, P, n, lastP, lnp, color, in_dir, lld=False, bug=None):
    """rmis_last_pdf (getLast_pdf)"""
    ov = lastP - P
    p = E.pdf(M, n, in_dir, _unit(ov))
    with np.errstate(all="ignore"):
        area = p / _dot(ov, ov) * (1.0 if bug == "last_normal_projection dropped from LL_pdf" else lnp)
    return np.where(lld, p, area) * rr_of(color)


def _flux_multiplier(E, M, n, color, in_dir, out_dir, div_on):
    """rmis_flux_multiplier (getFluxMultiplier)"""
    with np.errstate(all="ignore"):
        f = _div(M, E.eval(M, n, in_dir, out_dir), n, out_dir, div_on)
        return f * np.abs(_dot(n, out_dir))[..., None] / E.pdf(M, n, in_dir, out_dir)[..., None] / rr_of(color)[..., None]


def _get_pdf(E, M, P, n, color, endP, endN, in_dir, bug=None):
    """rmis_get_pdf (getPdf)"""
    ov = endP - P
    od = _unit(ov)
    with np.errstate(all="ignore"):
        p = E.pdf(M, n, in_dir, od) / _dot(ov, ov) * np.abs(_dot(od, endN))
    return p * (1.0 if bug == "rr dropped" else rr_of(color))


def _gamma(gh, e, l, bug=None):
    e, l = np.asarray(e, np.int64), np.asarray(l, np.int64)
    assert ((e >= 0) & (e < NUM_SUBSPACE) & (l >= 0) & (l < NUM_SUBSPACE)).all(), "a label outside [0, NUM_SUBSPACE)"
    return gh[l, e] if bug == "Gamma indices transposed" else gh[e, l]


def _invalid(v):
    with np.errstate(invalid="ignore"):
        return ((v > INVALID) | np.isnan(v)).any(-1)


def tree_labels(tree, P, n):
    """labels of (position, normal) under a classifier without direction nodes (the direction handed over is the normal)"""
    from oracle import binding as ob
    return ob.tree_index(tree, np.concatenate([np.asarray(P, np.float32), np.asarray(n, np.float32), np.asarray(n, np.float32)], 1)).astype(np.int64)


def has_direction_nodes(tree):
    return bool(((tree["leaf"] == 0) & (tree["type"] == 2)).any())


# ---- the connection ------------------------------------------------------------------------------------------------------------
def connect_labels(tup, a, b, form, lsub):
    """(light label of a, eye label of b) as the form takes them"""
    et, lt = tup[0], tup[1]
    assert not (has_direction_nodes(et) or has_direction_nodes(lt))
    if form == "reference":
        return tree_labels(lt, a["position"], a["normal"]), tree_labels(et, b["position"], b["normal"])
    stored = (b["pad"] & np.uint32(0xffff)).astype(np.int64) - 1
    descent = ((stored < 0) | (stored >= NUM_SUBSPACE)) & (b["depth"] != 0)
    eye = np.where(descent, tree_labels(et, b["position"], b["normal"]), np.clip(stored, 0, NUM_SUBSPACE - 1))   # (an emitter's is never read)
    return np.asarray(lsub, np.int64), eye


def _connect(W, d, E, bug=None):
    """The module docstring's connect() for the records W, positions displaced by d = (dPa, dPb, dPla, dPlb)."""
    a, b, Ma, Mb, gh = W["a"], W["b"], W["Ma"], W["Mb"], W["gh"]
    env = W["form"] != "cached_plain"
    Pa, Pb = _f64(a["position"]) + d[0], _f64(b["position"]) + d[1]
    Pla, Plb = _f64(a["last_position"]) + d[2], _f64(b["last_position"]) + d[3]
    na, nb = _f64(a["normal"]), _f64(b["normal"])
    with np.errstate(all="ignore"):
        aflux, bflux, apdf, bpdf = _f64(a["flux"]), _f64(b["flux"]), _f64(a["pdf"]), _f64(b["pdf"])
        lflux = bflux / bpdf[:, None]
        cv = Pa - Pb
        r2 = _dot(cv, cv)
        c = cv / np.sqrt(r2)[:, None]
        LA, LB = _unit(Pla - Pa), _unit(Plb - Pb)
        origin = b["depth"] == 0
        sky = ((b["pad"] & np.uint32(LV_DIRECTION)) != 0) & env
        lld = ((b["pad"] & np.uint32(LV_LAST_DIRECTION)) != 0) & env
        nconn = 1.0 if bug == "CONNECTION_N dropped" else float(CONNECTION_N)
        wA = np.where(a["depth"] == 1, 0.0, _gamma(gh, a["last_zone_id"], W["light_label"], bug) * nconn)
        weight = _sum3(_gamma(gh, a["subspace_id"], b["subspace_id"], bug)[:, None] * lflux * nconn)
        R3, asp = _f64(a["rmis3"]), _f64(a["single_pdf"])
        brmis, bsp = _f64(b["rmis_pointer"]), _f64(b["single_pdf"])
        lnp_a, lnp_b = _f64(a["last_normal_projection"]), _f64(b["last_normal_projection"])

        # -- surface / emitter light vertex
        g_r = np.sqrt(r2) if bug == "1 / r^2 -> 1 / r" else r2
        G = np.abs(_dot(na, c)) * np.abs(_dot(nb, c)) / g_r
        fa = _div(Ma, E.eval(Ma, na, -c, LA), na, c, env)
        D_A_0 = R3 * _last_pdf(E, Ma, Pa, na, Pla, lnp_a, a["color"], -c, bug=bug)[:, None] * _flux_multiplier(E, Ma, na, a["color"], -c, LA, env) + wA[:, None]
        pdf_B = _get_pdf(E, Ma, Pa, na, a["color"], Pb, nb, LA, bug)
        # emitter
        behind = _dot(nb, -c) > 0.0
        if bug == "fb one-sided test flipped":
            behind = ~behind
        fb_o = np.where(behind, 0.0, 1.0)[:, None] * np.ones(3)
        pdfA_o = np.abs(_dot(nb, c)) / np.pi * np.abs(_dot(na, c)) / r2
        DA_o = _sum3(D_A_0 * (pdfA_o * np.pi)[:, None] * lflux / asp[:, None])
        DB_o = brmis * pdf_B / bsp
        # surface
        fb_s = _div(Mb, E.eval(Mb, nb, c, LB), nb, c, env)
        if bug == "pdf_A taken from the wrong vertex":   # getPdf(eye, ...) where getPdf(light, eye, LA) belongs
            pdfA_s = _get_pdf(E, Ma, Pa, na, a["color"], Pb, nb, LA)
        else:
            pdfA_s = _get_pdf(E, Mb, Pb, nb, b["color"], Pa, na, LB, bug)
        fm1 = _flux_multiplier(E, Mb, nb, b["color"], LB, c, env)
        DA_s = _sum3(D_A_0 * pdfA_s[:, None] * fm1 * lflux / asp[:, None])
        LL_B = _last_pdf(E, Mb, Pb, nb, Plb, lnp_b, b["color"], c, lld=lld, bug=bug)
        wB = _gamma(gh, W["eye_label"], b["last_zone_id"], bug) * _f64(b["last_lum"]) * nconn
        DB_s = (brmis * LL_B + wB) * pdf_B / bsp
        D_A, D_B, fb = np.where(origin, DA_o, DA_s), np.where(origin, DB_o, DB_s), np.where(origin[:, None], fb_o, fb_s)
        w = weight / (weight + D_A + D_B)
        through = aflux * bflux * fa * fb * G[:, None] / (apdf * bpdf)[:, None]
        s_a, s_b = _dot(na, -c), _dot(nb, c)
        null = (s_a <= 0.0) | (s_b < 0.0)

        # -- the sky direction arm
        if sky.any():
            cs = -nb
            up = _dot(na, cs)
            f = E.eval(Ma, na, LA, cs) * up[:, None]
            LL_A = _last_pdf(E, Ma, Pa, na, Pla, lnp_a, a["color"], _unit(Pb - Pa), bug=bug)
            D0 = R3 * LL_A[:, None] * _flux_multiplier(E, Ma, na, a["color"], cs, LA, True) + wA[:, None]
            pdfA = W["project_pdf"] * np.abs(_dot(nb, na))
            DA_d = _sum3(D0 * (pdfA * float(np.float32(1.0 / W["project_pdf"])))[:, None] * lflux / asp[:, None])
            pdfB = E.pdf(Ma, na, LA, cs) * (1.0 if bug == "rr dropped" else rr_of(a["color"]))
            DB_d = brmis * pdfB / bsp
            w_d = np.where(up > 0.0, weight / (weight + DA_d + DB_d), 0.0)
            th_d = np.where((up > 0.0)[:, None], aflux / apdf[:, None] * f * bflux / bpdf[:, None], 0.0)
            w, through = np.where(sky, w_d, w), np.where(sky[:, None], th_d, through)
            null, s_a, s_b = np.where(sky, ~(up > 0.0), null), np.where(sky, up, s_a), np.where(sky, 1.0, s_b)
    return dict(w=w, through=through, null=null, s_a=s_a, s_b=s_b, sky=sky)


def _graze(P, lastP, n, traced):
    """1 / cosine of the ray that arrived at a traced vertex, in [1, 1e4] (lvc_audit: a hit point's rounding grows with it)"""
    with np.errstate(all="ignore"):
        c = np.abs(_dot(n, _unit(P - lastP)))
        return np.where(traced, np.clip(1.0 / np.nan_to_num(c, nan=1.0), 1.0, 1e4), 1.0)[:, None]


def _spread(x, base):
    with np.errstate(all="ignore"):
        k = np.abs(x - base).max(-1) / (np.abs(base).max(-1) + 1e-30) if base.ndim > 1 else np.abs(x - base) / (np.abs(base) + 1e-30)
        # a base that is NaN is 0 / 0 of exact zeros (a coplanar pair in a zero-handled cell): FP32 has the same zeros, and the
        # record is judged as it stands (NaN equals NaN, and nothing else)
        k = np.where(np.isnan(base).any(-1) if base.ndim > 1 else np.isnan(base), 0.0, k)
        # ... and a base that is exactly 0 is a product with an exact zero in it (a coplanar pair: both cosines 0; Eval below the
        # surface): nothing is relative to it, and FP32 returns the same 0
        k = np.where((base == 0).all(-1) if base.ndim > 1 else base == 0, 0.0, k)
    return np.where(np.isnan(k), np.inf, k)


def connect(scene, tup, a, b, form="reference", lsub=None, project_pdf=0.0, extent=None, bug=None, kappa=True):
    """The definition's answer for the pairs (a, b): dict(w, through, null, s_a, s_b, k_w, k_through).  The VALUE the device must
    return is value_of(through, its own w)."""
    assert form in FORMS
    n = len(a)
    lsub = np.zeros(n, np.int64) if lsub is None else lsub
    ll, el = connect_labels(tup, a, b, form, lsub)
    W = dict(a=a, b=b, form=form, Ma=materials(scene, a["material_id"], a["color"]), gh=gamma_hat(tup[2], tup[3]),
             Mb=materials(scene, np.where(b["depth"] == 0, 0, b["material_id"]), b["color"]), light_label=ll, eye_label=el, project_pdf=project_pdf)
    zero = np.zeros((n, 3))
    out = _connect(W, (zero, zero, zero, zero), _Lens(), bug)
    out["k_w"], out["k_through"] = np.zeros(n), np.zeros(n)
    if not kappa:
        return out
    extent = float(np.linalg.norm(scene.vertices.max(0) - scene.vertices.min(0))) if extent is None else extent
    Pa, Pb = _f64(a["position"]), _f64(b["position"])
    ua = _ulp(Pa, extent) * _graze(Pa, _f64(a["last_position"]), _f64(a["normal"]), np.ones(n, bool))
    ub = _ulp(Pb, extent) * _graze(Pb, _f64(b["last_position"]), _f64(b["normal"]), b["depth"] > 0)
    ula, ulb = _ulp(_f64(a["last_position"]), extent), _ulp(_f64(b["last_position"]), extent)
    rng = np.random.default_rng(0x5EED)
    for k in range(N_PATTERNS):
        sg = rng.choice([-1.0, 1.0], size=(4, 1, 3))
        pr = _connect(W, (sg[0] * ua, sg[1] * ub, sg[2] * ula, sg[3] * ulb), _lens(k), bug)
        out["k_w"] = np.maximum(out["k_w"], _spread(pr["w"], out["w"]))
        out["k_through"] = np.maximum(out["k_through"], _spread(pr["through"], out["through"]))
    # a cosine of two FP32 unit vectors carries an absolute error of an ulp of 1 whatever its size: G, pdf_A and pdf_B are
    # proportional to the connection's two cosines
    with np.errstate(all="ignore"):
        graze = EPS32 * (1.0 / np.abs(out["s_a"]) + np.where(out["sky"], 0.0, 1.0 / np.abs(out["s_b"])))
    live = (out["through"] != 0).any(-1)
    out["k_through"] = out["k_through"] + np.where(live, graze, 0.0)
    out["k_w"] = out["k_w"] + np.where(live & ~np.isnan(out["w"]) & (out["w"] != 0), graze, 0.0)
    return out


def value_of(through, w):
    """through x w, or 0 where ISINVALIDVALUE rejects it"""
    with np.errstate(all="ignore"):
        v = through * _f64(w)[:, None]
    return np.where(_invalid(v)[:, None], 0.0, v)


def audit_connect(scene, tup, a, b, got_rgb, got_w, got_null=None, judge_value=None, **kw):
    """{check: Check} of the outputs of CONNECT (rgb, weight, null flag) against connect().  judge_value: the records whose value and
    weight are judged (default all); the sign and zero checks cover every record."""
    D = connect(scene, tup, a, b, **kw)
    n = len(a)
    idx = np.arange(n)
    jv = np.ones(n, bool) if judge_value is None else judge_value
    got_rgb = np.asarray(got_rgb)
    with np.errstate(all="ignore"):
        raw = D["through"] * _f64(got_w)[:, None]
        top = np.where(np.isnan(raw).any(-1), np.inf, np.abs(raw).max(-1))
        # within the bar of the rejection threshold either answer, the product or 0, is the definition's
        edge = np.abs(top - INVALID) <= INVALID * (BARS["connect value"][1] + C_KAPPA * D["k_through"])
    want = np.where(_invalid(raw)[:, None], 0.0, raw)
    e_v = rel(got_rgb, want)
    e_v = np.where(edge, np.minimum(e_v, np.where((got_rgb == 0).all(-1), 0.0, rel(got_rgb, raw))), e_v)
    # with the sky below a's surface the direction arm returns before it has a weight (the harness reports 0, the reference's
    # connection_direction_lightSource a number nothing multiplies): the value is an exact zero, the weight is not judged
    jw = jv & ~(D["sky"] & D["null"])
    out = {"connect value": Check("connect value", idx[jv], e_v[jv], D["k_through"][jv]),
           "connect weight": Check("connect weight", idx[jw], rel(got_w, D["w"])[jw], D["k_w"][jw])}

    def clear_of_sign_change(s):     # an exact zero is exact on both sides; else the cosine is more than an FP32 ulp from its sign change
        return (np.abs(s) > SIGN_ULP) | (s == 0.0)
    clear = clear_of_sign_change(D["s_a"]) & clear_of_sign_change(D["s_b"])
    zero = (want == 0).all(-1) & ~edge & clear
    out["connect: exact zeros"] = Check("connect: exact zeros", idx[zero], (got_rgb[zero] != 0).any(-1).astype(float))
    if got_null is not None:
        gn = np.asarray(got_null) != 0
        out["connect: null flag"] = Check("connect: null flag", idx[clear], (gn != D["null"])[clear].astype(float))
        out["connect: null => value 0"] = Check("connect: null => value 0", idx[gn], (got_rgb[gn] != 0).any(-1).astype(float))
    out["_def"] = D
    return out


# ---- the eye step ----------------------------------------------------------------------------------------------------------------
def roulette_draw(seed):
    """the fourth LCG draw of the input seed (three go to Sample), and the seed afterwards"""
    _, _, _, s = B.draws(seed)
    s = (np.uint64(B.LCG_A) * s.astype(np.uint64) + np.uint64(B.LCG_C)) & np.uint64(B.M32 - 1)
    return (s & np.uint64(0xFFFFFF)).astype(np.float64) / (1 << 24), s.astype(np.uint32)


def _walk_terms(W, E, d, bug=None):
    """What an eye vertex l hands to whatever its next segment meets at Pm: LL_l, fm_l, w_l of the recursion (rmis.h:189-207)"""
    l, Ml, gh = W["l"], W["Ml"], W["gh"]
    env = W["form"] != "cached_plain"
    Pl, Pll, Pm = _f64(l["position"]) + d[0], _f64(l["last_position"]) + d[1], W["Pm"] + d[2]
    nl = _f64(l["normal"])
    in_dir = W["in_dir"] if W.get("in_dir") is not None else _unit(Pm - Pl)
    LL = _last_pdf(E, Ml, Pl, nl, Pll, _f64(l["last_normal_projection"]), l["color"], in_dir, bug=bug)
    fm = _flux_multiplier(E, Ml, nl, l["color"], in_dir, _unit(Pll - Pl), env)
    nconn = 1.0 if bug == "CONNECTION_N dropped" else float(CONNECTION_N)
    wl = np.where(l["depth"] == 1, 0.0, _gamma(gh, np.where(l["depth"] <= 1, 0, l["last_zone_id"]), W["light_label"], bug) * nconn)
    return LL, fm, wl, Pl, Pll, Pm


def _eye_step(W, E, d, bug=None):
    l, m = W["l"], W["m"]
    nl, nm, dr = _f64(l["normal"]), _f64(m["normal"]), W["dir"]
    t = W["t"] * (1.0 + d[3])
    with np.errstate(all="ignore"):
        cos_l = np.abs(_dot(nl, dr))
        pdf_g = np.abs(_dot(nm, dr)) * cos_l / (t if bug == "1 / r^2 -> 1 / r" else t * t)
        origin = l["depth"] == 0
        lflux = _f64(l["flux"])
        flux = np.where(origin[:, None], lflux * pdf_g[:, None], W["next_flux"] * lflux * pdf_g[:, None])
        single_pdf = W["next_single_pdf"] * pdf_g / cos_l
        LL, fm, wl, _, _, _ = _walk_terms(W, E, d, bug)
        rmis3 = np.where(origin[:, None], 0.0, (_f64(l["rmis3"]) * LL[:, None] * fm + wl[:, None]) / _f64(l["single_pdf"])[:, None])
        env = W["form"] != "cached_plain"
        s = W["new_dir"]
        nf = _div(W["Mm"], E.eval(W["Mm"], nm, -dr, s), nm, s, env)
        npdf = E.pdf(W["Mm"], nm, -dr, s)
        nsp = npdf * (1.0 if bug == "rr dropped" else rr_of(m["color"]))
    return dict(flux=flux, single_pdf=single_pdf, lnp=cos_l, rmis3=rmis3, next_flux=nf, next_single_pdf=nsp, next_pdf=npdf)


def _patterns(fn, n, ulps, keys, n_extra=1):
    """base = fn(zeros), kappa[key] = the largest relative change over N_PATTERNS sign patterns of the displacements `ulps`"""
    zero = [np.zeros((n, 3))] * len(ulps) + [0.0] * n_extra
    base = fn(zero, _Lens())
    kap = {k: np.zeros(n) for k in keys}
    rng = np.random.default_rng(0x5EED)
    for k in range(N_PATTERNS):
        sg = rng.choice([-1.0, 1.0], size=(len(ulps), 1, 3))
        pr = fn([sg[i] * u for i, u in enumerate(ulps)] + [EPS32 * (1 if k % 2 else -1)] * n_extra, _lens(k))
        for key in keys:
            kap[key] = np.maximum(kap[key], np.abs(pr[key] - base[key]) if key == "lnp" else _spread(pr[key], base[key]))
    return base, kap


def eye_step_labels(tup, last, form, lsub):
    if form == "reference":
        return tree_labels(tup[1], last["position"], last["normal"])
    return np.asarray(lsub, np.int64)


def audit_eye_step(scene, tup, rec, out, form="reference", lsub=None, got_lsub=None, bug=None):
    """{check: Check} of the surface-vertex records of EYE_STEP (rec: EYE_STEP_IN_DTYPE, out: EYE_STEP_OUT_DTYPE) against
    eye_vertex(); the emitter hits among them go to audit_emitter_hit."""
    sel = np.nonzero(out["kind"] == 1)[0]
    l, m, o = rec["last"][sel], out["mid"][sel], out[sel]
    n = len(sel)
    lsub = np.zeros(len(rec), np.int64) if lsub is None else np.asarray(lsub)
    extent = float(np.linalg.norm(scene.vertices.max(0) - scene.vertices.min(0)))
    lmat = np.where(l["depth"] == 0, 0, l["material_id"])
    W = dict(l=l, m=m, form=form, Ml=materials(scene, lmat, l["color"]), Mm=materials(scene, m["material_id"], m["color"]),
             gh=gamma_hat(tup[2], tup[3]), light_label=eye_step_labels(tup, l, form, lsub[sel]), Pm=_f64(m["position"]),
             dir=_f64(rec["dir"][sel]), t=_f64(o["t_hit"]), next_flux=_f64(rec["next_flux"][sel]), next_single_pdf=_f64(rec["next_single_pdf"][sel]),
             new_dir=_f64(o["dir"]))
    Pl = _f64(l["position"])
    ulps = [_ulp(Pl, extent) * _graze(Pl, _f64(l["last_position"]), _f64(l["normal"]), l["depth"] > 0), _ulp(_f64(l["last_position"]), extent),
            _ulp(W["Pm"], extent) * np.clip(1.0 / np.maximum(np.abs(_dot(_f64(m["normal"]), W["dir"])), 1e-4), 1.0, 1e4)[:, None]]
    keys = ("flux", "single_pdf", "lnp", "rmis3", "next_flux", "next_single_pdf")
    base, kap = _patterns(lambda d, E: _eye_step(W, E, d, bug), n, ulps, keys)
    C = {}

    def add(name, mask, err, kappa=None, cap=0.0):
        C[name] = Check(name, sel[mask], np.asarray(err, np.float64)[mask], None if kappa is None else kappa[mask], cap)
    every = np.ones(n, bool)
    add("eye flux", every, rel(m["flux"], base["flux"]), kap["flux"])
    add("eye single_pdf", every, rel(m["single_pdf"], base["single_pdf"]), kap["single_pdf"])
    add("eye pdf", every, rel(m["pdf"], _f64(l["pdf"]) * _f64(m["single_pdf"])), np.zeros(n))
    add("eye last_normal_projection", every, np.abs(_f64(m["last_normal_projection"]) - base["lnp"]), kap["lnp"])
    add("eye rmis3", every, rel(m["rmis3"], base["rmis3"]), kap["rmis3"])
    add("eye: rmis3 is 0 at depth 1", l["depth"] == 0, (m["rmis3"] != 0).any(-1).astype(float))
    add("eye: last_position, depth, last_zone_id", every,
        ((m["last_position"] != l["position"]).any(-1) | (m["depth"] != l["depth"] + 1) | (m["last_zone_id"] != l["subspace_id"])).astype(float))
    add("eye: subspace label", every, (m["subspace_id"] != tree_labels(tup[0], m["position"], m["normal"])).astype(float), cap=LABEL_CAP)
    if got_lsub is not None:
        want = np.where((m["depth"] == 1) | (form == "reference"), 0, tree_labels(tup[1], m["position"], m["normal"]))
        add("eye: lsub label", every, (np.asarray(got_lsub)[sel] != want).astype(float), cap=LABEL_CAP)
    # the path ends where Pdf is not positive or the roulette number exceeds rr: rr and the number are exact; Pdf <= 0 only below the surface
    r, seed_after = roulette_draw(rec["seed"][sel])
    done = ~(base["next_pdf"] > 0.0) | (r > rr_of(m["color"]))
    if (rec["flags"][sel] & 1).any():
        done |= ((rec["flags"][sel] & 1) != 0) & (o["next_flux"] == 0).all(-1)
    add("eye: seed", every, (o["seed"] != seed_after).astype(float))        # an integer function of the input seed: exact
    add("eye: done", every, ((o["done"] != 0) != done).astype(float), cap=LABEL_CAP)   # (Pdf > 0 sits on a rounding boundary)
    add("next flux", every, rel(o["next_flux"], base["next_flux"]), kap["next_flux"])
    alive = (o["done"] == 0) & ~done
    add("next single_pdf", alive, rel(o["next_single_pdf"], base["next_single_pdf"]), kap["next_single_pdf"])
    C["_def"] = dict(sel=sel, base=base, kappa=kap)
    return C


def light_of_hit(lights, P, tol):
    """(light index, patch label, the light's normal there) of points on quad and mesh lights (lvc_audit's origin checks, the other
    way round); a mesh light's normal is the hit triangle's own"""
    from tests.lvc_audit import _locate
    best, lab, dist, nrm = np.full(len(P), -1), np.zeros(len(P), np.int64), np.full(len(P), np.inf), np.zeros((len(P), 3))
    for j, L in enumerate(lights):
        if L["type"] == 0:
            w = P - L["corner"]
            uu, uv, vv = _dot(L["u"], L["u"]), _dot(L["u"], L["v"]), _dot(L["v"], L["v"])
            den = uu * vv - uv * uv
            r1 = (vv * _dot(w, L["u"]) - uv * _dot(w, L["v"])) / den
            r2 = (uu * _dot(w, L["v"]) - uv * _dot(w, L["u"])) / den
            off = np.abs(_dot(w, L["normal"])) + 10.0 * np.maximum(np.maximum(-r1, r1 - 1), np.maximum(-r2, r2 - 1)).clip(0)
            xb = np.clip(np.floor(r1 * L["div"]), 0, L["div"] - 1).astype(np.int64)
            yb = np.clip(np.floor(r2 * L["div"]), 0, L["div"] - 1).astype(np.int64)
            cell, n_j = xb * L["div"] + yb, np.broadcast_to(L["normal"], (len(P), 3))
        elif L["type"] == 2:
            off, which, nn = _locate(P, L["tris"], tol)
            cell, n_j = np.asarray(L["patch"], np.int64)[which], nn[which]
        else:
            continue
        take = off < dist
        best, dist = np.where(take, j, best), np.where(take, off, dist)
        lab, nrm = np.where(take, NUM_SUBSPACE - (L["base"] + cell) - 1, lab), np.where(take[:, None], n_j, nrm)
    return best, lab, nrm


def _light_hit(W, E, d, bug=None):
    """emitter_hit() / sky_miss(): radiance and 1 / RMIS_pointer of the records W"""
    l, Ml = W["l"], W["Ml"]
    nl, dr = _f64(l["normal"]), W["dir"]
    sky = W["sky"]
    with np.errstate(all="ignore"):
        LL, fm, wl, Pl, Pll, Pm = _walk_terms(W, E, d, bug)
        cos_l = np.abs(_dot(nl, dr))
        origin = l["depth"] == 0
        Le, ln, lpdf = W["Le"], W["ln"], W["light_pdf"]
        if sky:
            pdf_g = cos_l
            pdf_A, fmB = W["project_pdf"] * np.abs(_dot(-dr, nl)), float(np.float32(1.0 / W["project_pdf"]))
            pdf_B = E.pdf(Ml, nl, _unit(Pll - Pl), dr) * (1.0 if bug == "rr dropped" else rr_of(l["color"]))
        else:
            t = W["t"] * (1.0 + d[3])
            pdf_g = np.abs(_dot(ln, dr)) * cos_l / (t if bug == "1 / r^2 -> 1 / r" else t * t)
            Pm = Pm + (W["t"] * d[3])[:, None] * dr          # (the hit point is rebuilt from the reported t)
            cv = Pl - Pm
            c = _unit(cv)
            pdf_A, fmB = np.abs(_dot(ln, c)) / np.pi * np.abs(_dot(nl, c)) / _dot(cv, cv), np.pi
            pdf_B = _get_pdf(E, Ml, Pl, nl, l["color"], Pm, ln, _unit(Pll - Pl), bug)
        lflux = _f64(l["flux"])
        flux = np.where(origin[:, None], lflux, W["next_flux"] * lflux) * pdf_g[:, None] * Le
        pdf = _f64(l["pdf"]) * (W["next_single_pdf"] * pdf_g / cos_l)
        lf = Le / lpdf[:, None]
        nconn = 1.0 if bug == "CONNECTION_N dropped" else float(CONNECTION_N)
        D_A = _sum3((_f64(l["rmis3"]) * LL[:, None] * fm + wl[:, None]) * (pdf_A * fmB)[:, None] * lf / _f64(l["single_pdf"])[:, None])
        weight = _sum3(_gamma(W["gh"], np.where(origin, 0, l["subspace_id"]), W["label"], bug)[:, None] * lf * nconn)
        R = np.where(origin, 1.0, 1.0 + (weight + D_A) / pdf_B * lpdf)
        ans = flux / pdf[:, None] / R[:, None]
        ans = np.where(_invalid(ans)[:, None], 0.0, ans)
        if not sky:
            ans = np.where((_dot(dr, ln) > 0.0)[:, None], 0.0, ans)
    return dict(value=ans, w=1.0 / R)


def audit_emitter_hit(scene, tup, rec, out, form="reference", lsub=None, env=None, bug=None):
    """{check: Check} of the emitter hits (kind 2 and 3; quad and mesh lights) of EYE_STEP records against emitter_hit()."""
    sel = np.nonzero((out["kind"] == 2) | (out["kind"] == 3))[0]
    l, o = rec["last"][sel], out[sel]
    n = len(sel)
    lsub = np.zeros(len(rec), np.int64) if lsub is None else np.asarray(lsub)
    lights = scene_lights(scene, env)
    extent = float(np.linalg.norm(scene.vertices.max(0) - scene.vertices.min(0)))
    dr, t = _f64(rec["dir"][sel]), _f64(o["t_hit"])
    Pm = _f64(l["position"]) + t[:, None] * dr
    li, label, ln = light_of_hit(lights, Pm, 64.0 * float(np.spacing(np.float32(extent))))
    assert (li >= 0).all()
    n_lights = len(lights)
    W = dict(l=l, form=form, Ml=materials(scene, np.where(l["depth"] == 0, 0, l["material_id"]), l["color"]), gh=gamma_hat(tup[2], tup[3]),
             light_label=eye_step_labels(tup, l, form, lsub[sel]), Pm=Pm, dir=dr, t=t, sky=False, label=label,
             next_flux=_f64(rec["next_flux"][sel]), next_single_pdf=_f64(rec["next_single_pdf"][sel]),
             Le=np.array([_f64(lights[j]["emission"]) for j in li]).reshape(n, 3), ln=ln,
             light_pdf=np.array([float(np.float32(1.0 / (np.float32(lights[j]["area"]) * n_lights))) for j in li]))
    Pl = _f64(l["position"])
    ulps = [_ulp(Pl, extent) * _graze(Pl, _f64(l["last_position"]), _f64(l["normal"]), l["depth"] > 0), _ulp(_f64(l["last_position"]), extent),
            _ulp(Pm, extent) * np.clip(1.0 / np.maximum(np.abs(_dot(W["ln"], dr)), 1e-4), 1.0, 1e4)[:, None]]
    base, kap = _patterns(lambda d, E: _light_hit(W, E, d, bug), n, ulps, ("value",))
    back = _dot(dr, W["ln"]) > 0.0
    C = {"emitter radiance": Check("emitter radiance", sel, rel(o["emit"], base["value"]), kap["value"]),
         "emitter: front / back": Check("emitter: front / back", sel, ((o["kind"] == 3) != back).astype(float)),
         "emitter: nothing from behind": Check("emitter: nothing from behind", sel[back], (o["emit"][back] != 0).any(-1).astype(float)),
         "_def": dict(sel=sel, base=base, kappa=kap)}
    return C


def audit_sky_miss(scene, tup, last, next_flux, next_single_pdf, dirs, got_rgb, got_w, got_label, env, form="reference", lsub=None, bug=None):
    """{check: Check} of SKY_MISS records against sky_miss()."""
    n = len(last)
    lsub = np.zeros(n, np.int64) if lsub is None else np.asarray(lsub)
    lights = scene_lights(scene, env)
    extent = float(np.linalg.norm(scene.vertices.max(0) - scene.vertices.min(0)))
    dr = _f64(dirs)
    pdf, edge = env_ref.env_pdf(lights[-1]["raster"], dr)
    label, ledge = env_ref.env_label(dr, lights[-1]["div"])
    W = dict(l=last, form=form, Ml=materials(scene, np.where(last["depth"] == 0, 0, last["material_id"]), last["color"]), gh=gamma_hat(tup[2], tup[3]),
             light_label=eye_step_labels(tup, last, form, lsub), Pm=_f64(last["position"]), in_dir=dr, dir=dr, sky=True, label=label,
             next_flux=_f64(next_flux), next_single_pdf=_f64(next_single_pdf), Le=env_ref.env_color(lights[-1]["raster"], dr), ln=-dr,
             light_pdf=pdf / len(lights), project_pdf=1.0 / (np.pi * lights[-1]["r"] ** 2))
    Pl = _f64(last["position"])
    ulps = [_ulp(Pl, extent) * _graze(Pl, _f64(last["last_position"]), _f64(last["normal"]), last["depth"] > 0), _ulp(_f64(last["last_position"]), extent), np.zeros((n, 3))]
    base, kap = _patterns(lambda d, E: _light_hit(W, E, d, bug), n, ulps, ("value", "w"))
    u64, v64 = env_ref.dir2uv(dr)
    contrast, big = env_ref.local_contrast(env_ref.texture(lights[-1]["raster"]), u64, v64)
    kap["value"] = kap["value"] + (SKY_UV * contrast + 2e-6 * big) / (np.abs(W["Le"]).max(-1) + 1e-30)     # env_color at an FP32 (u, v): lvc_audit's origin flux
    idx = np.arange(n)
    inside = (edge >= 1e-4) & (ledge >= 1e-4)          # within 1e-4 texel / cell of a border FP32 (u, v) may read the other one: counted, capped
    out = {} if got_rgb is None else {"sky value": Check("sky value", idx[inside], rel(got_rgb, base["value"])[inside], kap["value"][inside])}
    return {**out,
            "sky weight": Check("sky weight", idx[inside], rel(got_w, base["w"])[inside], kap["w"][inside]),
            "sky: within 1e-4 of a texel or cell border, not judged": Check("sky: within 1e-4 of a texel or cell border, not judged", idx, (~inside).astype(float), cap=LABEL_CAP),
            "sky: label": Check("sky: label", idx[inside], (np.asarray(got_label)[inside] != label[inside]).astype(float)),
            "_def": dict(base=base, kappa=kap)}


def figures(results, c_kappa=None):
    """{check: (99.9 % quantile, maximum of max(err - c kappa, 0) over the well-conditioned records, number of ill-conditioned ones)}:
    what the bars are a margin over"""
    from tests.lvc_audit import ILL_KAPPA, POLE_KAPPA
    c_kappa = C_KAPPA if c_kappa is None else c_kappa
    out = {}
    for name, c in results.items():
        if name.startswith("_") or c.kappa is None or not len(c.err):
            continue
        slack = c_kappa * c.kappa
        ill = ~(np.where(slack >= POLE_KAPPA, np.inf, slack) <= ILL_KAPPA)
        x = np.maximum(c.err - slack, 0.0)[~ill]
        out[name] = (float(np.quantile(x, 0.999)) if len(x) else 0.0, float(x.max()) if len(x) else 0.0, int(ill.sum()))
    return out


# ---- judging ---------------------------------------------------------------------------------------------------------------------
def judge(results, n, scenario, depth=None, report=print, bars=None):
    """lvc_audit.judge on the checks of an audit_* call over n records; records are named (index, depth)."""
    ids = np.zeros(n, dtype=[("path_id", "<i8"), ("depth", "<i8")])
    ids["path_id"] = np.arange(n)
    if depth is not None:
        ids["depth"] = depth
    return _judge(results, ids, scenario, bars=BARS if bars is None else bars, c_kappa=C_KAPPA, report=report)

