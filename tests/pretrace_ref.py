"""Float64 definition of the training records the "pretrace" pass writes, and the audit that holds a gathered record set to it (a
helper, not a test).

A gathered record set (Renderer.train_records() / Oracle.train_records()) describes its own paths: of a path with k = end_ind -
begin_ind nodes, node begin + j holds as a_* the eye surface vertex x_{j+1} and as b_* the vertex after it, the emitter point y for
the last node.  With the camera position that is the whole path eye, x_1 .. x_k, y and its normals, in stored FP32 values.  audit()
recomputes every other field from that path alone, in float64 numpy: no seeds, no lock-step with the oracle.  Written from
csrc/kernels_train.hip (k_pretrace, pretrace_build_path, the nv_* recursion) and csrc/eye_walk.h, quirks as they stand.

  materials     x_i lies on the scene triangle nearest to it (float64 point-to-triangle distance over ALL triangles); its material
                and colour are that triangle's (untextured scenes only).  Nearest triangle farther than LOCATE_TOL, or a triangle of
                another material within RIVAL_TOL: the vertex is UNLOCATED -- its path is counted (cap UNLOCATED_CAP), never passed.
                The stored normal must be +- the triangle's unit normal, turned against the arriving ray.
  eye chain     tests/connect_ref._eye_step, vertex by vertex, behind k_pretrace's camera vertex (normal = the ray direction,
                flux = pdf = singlePdf = 1): flux_i, singlePdf_i (roulette survival folded in), pdf_i = pdf_{i-1} singlePdf_i,
                brdf_div where the material asks for it.
  nVertex       the light-side vertex L_0 = (y, n_y, weight = Le, pdf = p_light, no direction, an emitter), extended one step per
                node towards the eye:  c = normalize(x - L.P), g = |c . n_x| |c . n_L| / r^2,
                  weight' = L.weight g                        behind an emitter
                          = L.weight g Eval(L; L.dir, c)      else                                   (nv_forward_light)
                  pdf'    = L.pdf |n_L . c| / pi |c . n_x| / r^2          behind an emitter
                          = L.pdf Pdf(L; L.dir, c) rr(L) |c . n_x| / r^2  else                      (nv_forward_light_pdf)
                  dir' = -c.  pdf' of an extended vertex reaches NO record field (only L_0.pdf does, through sample_pdf): the pdf arm
                of the light side is dead code of upstream's that the port keeps; the definition states it anyway.
  per node      node begin + j joins x_{j+1} with the light-side vertex L_{k-1-j}:  peak_pdf = pdf(x_{j+1}) sum_rgb L.weight;
                a_dir = normalize(x_j - x_{j+1}); b_dir = L.dir (zero at the emitter); label_a = j + 1 (the eye depth, exact);
                light_source = 1 on the last node only; b_position / b_normal = the next node's a_position / a_normal (exact);
                label_b = the emitter's patch (quads: the position inverted through corner, u, v, then light_reverse_sample's patch
                formula; mesh lights: the patch of the located triangle) on the last node, else the installed eye tree's label of
                (x_{j+2}, n, normalize(x_{j+1} - x_{j+2})) through the oracle's tree_index (pinned bit-exact elsewhere).
  per path      fix_pdf = pdf(x_k) Pdf(x_k; to x_{k-1}, to y) rr(x_k) |c . n_y| / r^2          (nv_forward_eye: the BSDF-sampled way to y)
                sample_pdf* = fix_pdf + pdf(x_k) p_light,  p_light = 1 / (A n_drawn): the density the next-event point is drawn from
                (A the light's area, n_drawn the lights it is drawn among: d16 -- with a sky, the area lights only)
                contri = flux(x_k) Le g(y, x_k) Eval(x_k; to x_{k-1}, to y), zeroed where sum_rgb contri / sample_pdf* is not finite
                stored sample_pdf = sample_pdf* / m, m = the kernel's acceptance count (rr_acc_accept: candidate number c replaces
                the kept one with probability 1 / (c_accepted + 1), an upstream quirk, not a uniform reservoir).  m is not stored:
                the audit takes m = round(sample_pdf* / stored), requires 1 <= m <= 2 k and judges |sample_pdf* / m - stored|.
                pixel_id = ((int)(width jx), (int)(height jy)) with normalize(x_1 - eye) ~ (2 jx - 1) U + (2 jy - 1) V + W.
Records within rounding of a patch border or a pixel border are BORDER records: counted (cap LABEL_CAP), never passed.

Conditioning, as tests/lvc_audit.py: every formula is evaluated again in N_PATTERNS fixed sign patterns with the positions moved by
+-1 FP32 ulp (taken at no less than a quarter of the scene's extent, over the cosine of the ray that arrived there, up to 1e4; the
emitter point y, mostly a sampled point, one ulp: the oracle's figures hold without more) and the
two directions handed to Eval / Pdf one ulp longer / shorter (connect_ref._lens); the largest change is the record's kappa and the
record is held to bar + C_KAPPA kappa, with lvc_audit's ILL_KAPPA, LOOSE_BAR, POLE_KAPPA, ILL_CAP rules (lvc_audit.judge does it)."""
from __future__ import annotations

import numpy as np

from tests import connect_ref as CR
from tests.lvc_audit import (C_KAPPA, EPS32, ILL_KAPPA, LABEL_CAP, N_PATTERNS, NUM_SUBSPACE, Check, _ulp, failed_checks, rr_of,  # noqa: F401 (failed_checks: for the tests)
                             scene_lights, scene_triangles)

UNLOCATED_CAP = 5e-3
BUGS = ("rr dropped from the pdf arm", "emitter cosine dropped from nv_forward_light_pdf", "Eval replaced by Pdf in the light arm",
        "light.pdf x n_lights", "nodes written in eye order", "peak_pdf from the vertex one step off", "m off by one")
# which field each seeded mistake must move (None: it reaches no record field -- the dead pdf arm, see the module docstring)
BUG_FIELD = {BUGS[0]: "fix_pdf", BUGS[1]: None, BUGS[2]: "peak_pdf", BUGS[3]: "sample_pdf", BUGS[4]: "peak_pdf", BUGS[5]: "peak_pdf",
             BUGS[6]: "sample_pdf"}

# ---- bars ---------------------------------------------------------------------------------------------------------------------
# field: (99.9 % bar, hard bar).  The 99.9 % bar is 4 x the ORACLE's largest 99.9 % quantile of max(err - C_KAPPA kappa, 0) over the
# well-conditioned records of the runs of tests/test_pretrace_definition_cpu.py (cornell_box, courtyard with its sky, simple_room(4);
# 64 x 64; num_core 4096 at paddings 10 / 3 / 2 and 4001 at padding 10; iterations 1 and 2 gathered), floored at 2e-6; the hard bar
# 4 x its largest maximum and no less than the 99.9 % bar.  Never from what the device gives.  tests/test_pretrace_definition_cpu.py holds
# both tables to the oracle's runs; tests/test_gpu_pretrace_definition.py prints the device's figures beside them.
ORACLE_FIGURES = {                         # field: the oracle's largest (99.9 % quantile, maximum) over the 12 runs; its ill-conditioned
    "peak_pdf": (4.12e-7, 6.27e-7),        # share of a run is at most 0.08 % (cap 0.5 %), unlocated vertices at most 0.32 % (cap 0.5 %),
    "fix_pdf": (1.36e-7, 4.29e-7),         # border records (patch, pixel) at most 0.02 % (cap 0.1 %)
    "sample_pdf": (4.03e-7, 6.76e-7),
    "contri": (3.27e-7, 8.46e-7),
    "a_dir": (1.01e-7, 1.02e-7),           # (absolute: a unit vector's component)
    "b_dir": (0.0, 0.0),                   # (the conditioning explains it all)
}
BARS = {
    "peak_pdf": (2e-6, 2.6e-6),
    "fix_pdf": (2e-6, 2e-6),
    "sample_pdf": (2e-6, 2.8e-6),
    "contri": (2e-6, 3.4e-6),
    "a_dir": (2e-6, 2e-6),
    "b_dir": (2e-6, 2e-6),
}
FLOAT_CHECKS = tuple(BARS)

_GH0 = None


def _gh0():
    global _GH0
    if _GH0 is None:
        _GH0 = np.zeros((NUM_SUBSPACE, NUM_SUBSPACE))
    return _GH0


_f64, _dot, _unit, rel = CR._f64, CR._dot, CR._unit, CR.rel


# ---- structural invariants (shared with tests/test_preprocess_cpu.py) ---------------------------------------------------------------
def check_invariants(paths, nodes, width, height, padding=10, emitter_label_min=None, sample_pdf_above_fix_pdf=False):
    """What every gathered record set satisfies whatever the scene (asserts)."""
    assert (paths["valid"] == 1).all() and (nodes["valid"] == 1).all()
    assert paths["begin_ind"][0] == 0 and (paths["begin_ind"][1:] == paths["end_ind"][:-1]).all() and paths["end_ind"][-1] == len(nodes)
    k = paths["end_ind"] - paths["begin_ind"]
    assert k.min() >= 1 and k.max() <= padding - 1          # eye surface vertices per path; the padding includes the camera
    assert (nodes["path_id"] == np.repeat(np.arange(len(paths)), k)).all()
    # label_a carries the eye depth 1..k until the trees exist (set_eye_depth)
    assert (nodes["label_a"] == np.concatenate([np.arange(1, kk + 1) for kk in k])).all()
    # the last node of a path joins the last eye vertex with the emitter vertex; the others have surface B vertices
    last = paths["end_ind"] - 1
    assert (nodes["light_source"][last] == 1).all()
    inner = np.ones(len(nodes), bool); inner[last] = False
    assert (nodes["light_source"][inner] == 0).all()
    if emitter_label_min is not None:
        assert (nodes["label_b"][last] >= emitter_label_min).all()
    assert np.isfinite(nodes["peak_pdf"]).all() and (nodes["peak_pdf"] >= 0).all()
    # sample_pdf is divided by the acceptance count m <= 2 k and fix_pdf is not (upstream's formula): sample_pdf >= fix_pdf holds only
    # where the next-event density dominates (the Cornell box; not under simple_room's large light)
    assert np.isfinite(paths["contri"]).all() and (paths["sample_pdf"].astype(np.float64) * (2 * k) * (1 + 1e-6) >= paths["fix_pdf"]).all()
    if sample_pdf_above_fix_pdf:
        assert (paths["sample_pdf"] >= paths["fix_pdf"]).all()
    assert (paths["pixel_id"] >= 0).all() and (paths["pixel_id"][:, 0] < width).all() and (paths["pixel_id"][:, 1] < height).all()
    return k


# ---- geometry ----------------------------------------------------------------------------------------------------------------------
def tri_distance(P, T, chunk=2048):
    """(n, t) float64 distances of the points P to the triangles T (t, 3, 3): the plane distance where the foot lies inside, else the
    least distance to the three edges."""
    a, e1, e2 = T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    nn = np.cross(e1, e2)
    nn = nn / np.linalg.norm(nn, axis=1, keepdims=True)
    d11, d12, d22 = _dot(e1, e1), _dot(e1, e2), _dot(e2, e2)
    den = d11 * d22 - d12 * d12
    out = np.empty((len(P), len(T)))
    for s in range(0, len(P), chunk):
        w = P[s:s + chunk, None, :] - a[None]
        h = np.abs(_dot(w, nn[None]))
        w1, w2 = _dot(w, e1[None]), _dot(w, e2[None])
        u, v = (d22 * w1 - d12 * w2) / den, (d11 * w2 - d12 * w1) / den
        inside = (u >= 0) & (v >= 0) & (u + v <= 1)
        best = np.full(h.shape, np.inf)
        for i0, i1 in ((0, 1), (1, 2), (2, 0)):
            p0, ed = T[:, i0], T[:, i1] - T[:, i0]
            q = P[s:s + chunk, None, :] - p0[None]
            tt = np.clip(_dot(q, ed[None]) / _dot(ed, ed)[None], 0.0, 1.0)
            r = q - tt[..., None] * ed[None]
            best = np.minimum(best, np.sqrt(_dot(r, r)))
        out[s:s + chunk] = np.where(inside, h, best)
    return out, nn


def camera_uvw(camera, aspect):
    """(eye, U, V, W) float64 of the FP32 frame the library builds from a scene's camera dict"""
    from __graft_entry__ import load_package
    U, V, W = load_package().api.camera_frame(camera["eye"], camera["lookat"], camera["up"], camera["fov"], aspect)
    return tuple(_f64(np.asarray(x, np.float32)) for x in (camera["eye"], U, V, W))


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def _predict(G, disp, E, bug=None):
    """Every formula of the module docstring for the n paths of one node count k.  G: X (n, k + 2, 3) positions eye, x_1..x_k, y; N
    their normals (N[:, 0] is rebuilt: the ray direction); mat, col of x_1..x_k at [:, 1..k]; Le, p_light; disp: displacement of X."""
    scene, k = G["scene"], G["k"]
    X = G["X"] + disp
    N = G["N"].copy()
    n = len(X)
    N[:, 0] = _unit(X[:, 1] - X[:, 0])
    zero3, ones = np.zeros((n, 3)), np.ones(n)
    M = [None] + [CR.materials(scene, G["mat"][:, i], G["col"][:, i]) for i in range(1, k + 1)]
    flux, pdf = [np.ones((n, 3))], [ones]
    l = dict(position=X[:, 0], normal=N[:, 0], depth=np.zeros(n, np.int64), flux=np.ones((n, 3)), rmis3=zero3, single_pdf=ones, last_position=X[:, 0],
             last_normal_projection=ones, color=zero3, last_zone_id=np.zeros(n, np.int64))
    Ml = CR.materials(scene, np.zeros(n, np.int64), zero3)
    nf, nsp = zero3, ones
    with np.errstate(all="ignore"):
        for i in range(1, k + 1):
            seg = X[:, i] - X[:, i - 1]
            t = np.sqrt(_dot(seg, seg))
            W = dict(l=l, m=dict(normal=N[:, i], color=G["col"][:, i]), form="reference", Ml=Ml, Mm=M[i], gh=_gh0(), light_label=np.zeros(n, np.int64),
                     Pm=X[:, i], dir=seg / t[:, None], t=t, next_flux=nf, next_single_pdf=nsp, new_dir=_unit(X[:, i + 1] - X[:, i]))
            r = CR._eye_step(W, E, [zero3, zero3, zero3, 0.0])
            flux.append(r["flux"]); pdf.append(pdf[-1] * r["single_pdf"])
            l = dict(position=X[:, i], normal=N[:, i], depth=np.full(n, i, np.int64), flux=r["flux"], rmis3=zero3, single_pdf=r["single_pdf"],
                     last_position=X[:, i - 1], last_normal_projection=r["lnp"], color=G["col"][:, i], last_zone_id=np.zeros(n, np.int64))
            Ml, nf, nsp = M[i], r["next_flux"], r["next_single_pdf"]
        # the light side, extended towards the eye
        peak, a_dir, b_dir = np.zeros((n, k)), np.zeros((n, k, 3)), np.zeros((n, k, 3))
        Lw, Lpdf, Lpos, Lnrm, Ldir, Lmat, Lcol = _f64(G["Le"]), G["p_light"] * ones, X[:, k + 1], N[:, k + 1], zero3, None, None
        for i in range(k):
            e = k - i
            pe = pdf[e - 1] if bug == "peak_pdf from the vertex one step off" else pdf[e]
            peak[:, e - 1] = pe * Lw.sum(-1)
            a_dir[:, e - 1] = _unit(X[:, e - 1] - X[:, e])
            b_dir[:, e - 1] = Ldir
            vec = X[:, e] - Lpos
            r2 = _dot(vec, vec)
            c = vec / np.sqrt(r2)[:, None]
            g = np.abs(_dot(c, N[:, e])) * np.abs(_dot(c, Lnrm)) / r2
            if Lmat is None:
                cos_e = 1.0 if bug == "emitter cosine dropped from nv_forward_light_pdf" else np.abs(_dot(Lnrm, c))
                w, p = Lw * g[:, None], Lpdf * cos_e / np.pi * np.abs(_dot(c, N[:, e])) / r2
            else:
                f = E.pdf(Lmat, Lnrm, Ldir, c)[:, None] if bug == "Eval replaced by Pdf in the light arm" else E.eval(Lmat, Lnrm, Ldir, c)
                w = Lw * g[:, None] * f
                p = Lpdf * E.pdf(Lmat, Lnrm, Ldir, c) * (1.0 if bug == "rr dropped from the pdf arm" else rr_of(Lcol)) * np.abs(_dot(c, N[:, e])) / r2
            Lw, Lpdf, Lpos, Lnrm, Ldir, Lmat, Lcol = w, p, X[:, e], N[:, e], -c, M[e], G["col"][:, e]
        if bug == "nodes written in eye order":
            peak = peak[:, ::-1]
        # the path
        vec = X[:, k + 1] - X[:, k]
        r2 = _dot(vec, vec)
        c = vec / np.sqrt(r2)[:, None]
        dk = _unit(X[:, k - 1] - X[:, k])
        ny = N[:, k + 1]
        rr = 1.0 if bug == "rr dropped from the pdf arm" else rr_of(G["col"][:, k])
        fix = pdf[k] * E.pdf(M[k], N[:, k], dk, c) * rr * np.abs(_dot(c, ny)) / r2
        p_light = G["p_light"] * (G["n_lights"] if bug == "light.pdf x n_lights" else 1.0)
        samp = fix + pdf[k] * p_light
        g0 = np.abs(_dot(c, N[:, k])) * np.abs(_dot(c, ny)) / r2
        contri = flux[k] * _f64(G["Le"]) * g0[:, None] * E.eval(M[k], N[:, k], dk, c)
        contri = np.where(np.isfinite(contri.sum(-1) / samp)[:, None], contri, 0.0)
    return dict(peak_pdf=peak, a_dir=a_dir, b_dir=b_dir, fix_pdf=fix, sample_star=samp, contri=contri, light_pdf_arm=Lpdf)


def audit(scene, tuple_, camera, width, height, paths, nodes, n_lights, n_drawn, env=None, bug=None):
    """scene: api.Scene (untextured); tuple_: get_subspace() of the tuple installed when the records were written (its eye tree labels
    the inner nodes); camera: (eye, U, V, W); n_lights: the scene's lights, the sky included; n_drawn: the lights the next-event
    candidate is drawn among; env: scene.environment of a scene with a sky; bug: one of BUGS, applied inside the definition.
    Returns {check: Check}; records are indexed paths first (0 .. len(paths) - 1), then nodes (len(paths) + node index)."""
    from oracle import binding as ob
    assert bug is None or bug in BUGS
    assert not any(int(m.get("albedo_tex", 0)) > 0 for m in scene.materials), "untextured scenes only"
    eye, U, V, Wv = (_f64(x) for x in camera)
    n_p, n_n = len(paths), len(nodes)
    lights = scene_lights(scene, env)
    tris, tri_mat, tri_emit = scene_triangles(scene, lights)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    extent = float(np.linalg.norm(hi - lo))
    ulp_e = float(np.spacing(np.float32(extent)))
    locate_tol, rival_tol = 64.0 * ulp_e, 1024.0 * ulp_e
    begin, end = paths["begin_ind"].astype(np.int64), paths["end_ind"].astype(np.int64)
    kk = end - begin
    out = {}
    node_path = np.repeat(np.arange(n_p), kk)
    j_of = np.arange(n_n) - begin[node_path]
    last = j_of == kk[node_path] - 1
    nidx = n_p + np.arange(n_n)

    # ---- exact fields
    out["label_a = eye depth"] = Check("label_a = eye depth", nidx, (nodes["label_a"] != j_of + 1).astype(float))
    out["light_source"] = Check("light_source", nidx, (nodes["light_source"] != last.astype(np.int32)).astype(float))
    inner = np.nonzero(~last)[0]
    link = (nodes["b_position"][inner] != nodes["a_position"][inner + 1]).any(1) | (nodes["b_normal"][inner] != nodes["a_normal"][inner + 1]).any(1)
    out["b vertex = next node's a vertex"] = Check("b vertex = next node's a vertex", nidx[inner], link.astype(float))

    # ---- locate every surface vertex
    A = _f64(nodes["a_position"])
    surf = np.nonzero(~tri_emit)[0]
    dist, tn = tri_distance(A, tris[surf])
    near = dist.argmin(1)
    dnear = dist[np.arange(n_n), near]
    mat = tri_mat[surf][near]
    other = np.where(tri_mat[surf][None, :] != mat[:, None], dist, np.inf).min(1)
    unlocated = (dnear > locate_tol) | (other <= rival_tol)
    out["unlocated vertices (their paths are not judged)"] = Check("unlocated vertices (their paths are not judged)", nidx, unlocated.astype(float), cap=UNLOCATED_CAP)
    path_ok = np.bincount(node_path, weights=unlocated, minlength=n_p) == 0
    base_col = np.array([np.asarray(m.get("color", (1, 1, 1)), np.float32) for m in scene.materials]).astype(np.float64)
    col = base_col[np.clip(mat, 0, len(base_col) - 1)]
    prevP = np.where((j_of == 0)[:, None], eye[None], np.roll(A, 1, axis=0))
    d_in = _unit(A - prevP)
    tnn = tn[near]
    tnn = np.where((_dot(tnn, d_in) > 0)[:, None], -tnn, tnn)
    n_err = np.maximum(np.abs(_f64(nodes["a_normal"]) - tnn).max(1) - 1e-6, 0.0)
    ok_n = path_ok[node_path]
    out["normal = the located triangle's, against the ray"] = Check("normal = the located triangle's, against the ray", nidx[ok_n], n_err[ok_n])

    # ---- the emitter point
    Y = _f64(nodes["b_position"][end - 1])
    li, lab_y, ln = CR.light_of_hit(lights, Y, locate_tol)
    y_bad = (li < 0)
    NY = _f64(nodes["b_normal"][end - 1])
    out["emitter normal"] = Check("emitter normal", np.arange(n_p), np.maximum(np.abs(NY - ln).max(1) - 1e-6, 0.0) + y_bad)
    li = np.clip(li, 0, len(lights) - 1)
    area = np.array([L.get("area", 1.0) for L in lights])[li]
    Le = np.array([_f64(L.get("emission", (0, 0, 0))) for L in lights])[li]
    # border: the patch label of a point within rounding of a patch border (quads: r1 div, r2 div near an integer)
    border_y = np.zeros(n_p, bool)
    for jl, L in enumerate(lights):
        s = np.nonzero(li == jl)[0]
        if L["type"] != 0 or not len(s):
            continue
        w = Y[s] - L["corner"]
        uu, uv, vv = _dot(L["u"], L["u"]), _dot(L["u"], L["v"]), _dot(L["v"], L["v"])
        den = uu * vv - uv * uv
        r1 = (vv * _dot(w, L["u"]) - uv * _dot(w, L["v"])) / den * L["div"]
        r2 = (uu * _dot(w, L["v"]) - uv * _dot(w, L["u"])) / den * L["div"]
        edge = np.minimum(np.abs(r1 - np.round(r1)), np.abs(r2 - np.round(r2)))
        interior = (np.round(r1) > 0) & (np.round(r1) < L["div"]) | (np.round(r2) > 0) & (np.round(r2) < L["div"])
        border_y[s] = (edge < 1e-5) & interior
    lb_last = nodes["label_b"][end - 1]
    out["label_b of the emitter: within 1e-5 patch of a border, not judged"] = Check("label_b of the emitter: within 1e-5 patch of a border, not judged", np.arange(n_p), border_y.astype(float), cap=LABEL_CAP)
    out["label_b of the emitter"] = Check("label_b of the emitter", np.arange(n_p)[~border_y], (lb_last != lab_y)[~border_y].astype(float))
    # inner nodes: the installed eye tree's label of the b vertex seen from the a vertex's side (a split within rounding: capped)
    if len(inner):
        bdir = _unit(A[inner] - A[inner + 1]).astype(np.float32)
        # (no tree installed yet: every surface vertex carries label 0)
        lab = ob.tree_index(tuple_[0], np.concatenate([nodes["b_position"][inner], nodes["b_normal"][inner], bdir], 1)) if len(tuple_[0]) else np.zeros(len(inner), np.int32)
        out["label_b of inner nodes"] = Check("label_b of inner nodes", nidx[inner], (nodes["label_b"][inner] != lab).astype(float), cap=LABEL_CAP)

    # ---- pixel id from x_1
    first = begin
    d1 = _unit(A[first] - eye[None])
    abc = np.linalg.solve(np.stack([U, V, Wv], 1), d1.T).T
    jx, jy = 0.5 * (abc[:, 0] / abc[:, 2] + 1.0), 0.5 * (abc[:, 1] / abc[:, 2] + 1.0)
    t1 = np.sqrt(_dot(A[first] - eye[None], A[first] - eye[None]))
    cos1 = np.maximum(np.abs(_dot(_f64(nodes["a_normal"][first]), d1)), 1e-4)
    # x_1 is a traced hit: a few ulps of its coordinates (lvc_audit's _ulp) over the arriving cosine; the FP32 ray direction a few of 1
    ptol = max(width, height) * (4.0 * _ulp(A[first], extent).max(1) / cos1 / t1 + 4.0 * EPS32)
    fx, fy = width * jx, height * jy
    border_p = (np.abs(fx - np.round(fx)) < ptol) | (np.abs(fy - np.round(fy)) < ptol)
    want_px = np.stack([np.floor(fx), np.floor(fy)], 1).astype(np.int64)
    out["pixel_id: within rounding of a pixel border, not judged"] = Check("pixel_id: within rounding of a pixel border, not judged", np.arange(n_p), border_p.astype(float), cap=LABEL_CAP)
    out["pixel_id"] = Check("pixel_id", np.arange(n_p)[~border_p], (paths["pixel_id"] != want_px).any(1)[~border_p].astype(float))

    # ---- the floating-point fields, one node count at a time
    res = {f: ([], [], []) for f in FLOAT_CHECKS}       # idx, err, kappa
    m_idx, m_err = [], []
    pred_all = {}
    for k in np.unique(kk):
        sel = np.nonzero((kk == k) & path_ok & ~y_bad)[0]
        n = len(sel)
        if not n:
            continue
        ni = begin[sel][:, None] + np.arange(k)[None, :]
        X = np.concatenate([np.broadcast_to(eye, (n, 1, 3)), A[ni], Y[sel][:, None]], 1)
        Nn = np.concatenate([np.zeros((n, 1, 3)), _f64(nodes["a_normal"])[ni], NY[sel][:, None]], 1)
        pad1 = np.zeros((n, 1), np.int64)
        G = dict(scene=scene, k=int(k), X=X, N=Nn, mat=np.concatenate([pad1, mat[ni]], 1), col=np.concatenate([np.zeros((n, 1, 3)), col[ni]], 1),
                 Le=Le[sel], p_light=1.0 / (area[sel] * n_drawn), n_lights=n_lights)
        base = _predict(G, np.zeros_like(X), CR._Lens(), bug)
        # conditioning
        with np.errstate(all="ignore"):
            seg_in = _unit(X[:, 1:] - X[:, :-1])
            graze = np.clip(1.0 / np.nan_to_num(np.abs(_dot(Nn[:, 1:], seg_in)), nan=1.0), 1.0, 1e4)
        ul = np.zeros_like(X)
        ul[:, 1:] = _ulp(X[:, 1:], extent) * graze[..., None]
        ul[:, k + 1] = _ulp(X[:, k + 1], extent)         # y: one ulp (module docstring)
        keys = ("peak_pdf", "fix_pdf", "sample_star", "contri", "a_dir", "b_dir")
        kap = {f: np.zeros(base[f].shape[:2] if f in ("peak_pdf", "a_dir", "b_dir") else (n,)) for f in keys}
        rng = np.random.default_rng(0x5EED)
        for pat in range(N_PATTERNS):
            sg = rng.choice([-1.0, 1.0], size=(1, k + 2, 3))
            pr = _predict(G, sg * ul, CR._lens(pat), bug)
            for f in keys:
                if f in ("a_dir", "b_dir"):
                    kap[f] = np.maximum(kap[f], np.abs(pr[f] - base[f]).max(-1))
                elif f == "peak_pdf":
                    kap[f] = np.maximum(kap[f], CR._spread(pr[f].reshape(-1), base[f].reshape(-1)).reshape(n, k))
                else:
                    kap[f] = np.maximum(kap[f], CR._spread(pr[f], base[f]))
        flat = ni.reshape(-1)
        res["peak_pdf"][0].append(n_p + flat); res["peak_pdf"][1].append(rel(nodes["peak_pdf"][flat], base["peak_pdf"].reshape(-1))); res["peak_pdf"][2].append(kap["peak_pdf"].reshape(-1))
        for f in ("a_dir", "b_dir"):
            res[f][0].append(n_p + flat); res[f][1].append(np.abs(_f64(nodes[f][flat]) - base[f].reshape(-1, 3)).max(-1)); res[f][2].append(kap[f].reshape(-1))
        res["fix_pdf"][0].append(sel); res["fix_pdf"][1].append(rel(paths["fix_pdf"][sel], base["fix_pdf"])); res["fix_pdf"][2].append(kap["fix_pdf"])
        res["contri"][0].append(sel); res["contri"][1].append(rel(paths["contri"][sel], base["contri"])); res["contri"][2].append(kap["contri"])
        with np.errstate(all="ignore"):
            stored = _f64(paths["sample_pdf"][sel])
            m = np.nan_to_num(np.round(base["sample_star"] / stored), nan=0.0, posinf=0.0)
            if bug == "m off by one":
                m = m + 1
            res["sample_pdf"][0].append(sel); res["sample_pdf"][1].append(rel(stored, base["sample_star"] / m)); res["sample_pdf"][2].append(kap["sample_star"])
        m_idx.append(sel); m_err.append(((m < 1) | (m > 2 * k)).astype(float))
        pred_all[int(k)] = dict(sel=sel, ni=ni, base=base, m=m)
    for f in FLOAT_CHECKS:
        i_, e_, k_ = (np.concatenate(x) if x else np.zeros(0) for x in res[f])
        out[f] = Check(f, i_.astype(np.int64), e_, k_)
    out["acceptance count 1 <= m <= 2 k"] = Check("acceptance count 1 <= m <= 2 k", np.concatenate(m_idx) if m_idx else [], np.concatenate(m_err) if m_err else [])
    out["_def"] = dict(pred=pred_all, n_paths=n_p, n_nodes=n_n, path_ok=path_ok, mat=mat)
    return out


def judge(results, scenario, bars=None, report=print):
    """Holds every check of audit() to its bar (lvc_audit.judge: bar + C_KAPPA kappa, the ILL_KAPPA / LOOSE_BAR / POLE_KAPPA rules,
    ILL_CAP, the caps of the counted exemptions).  Returns dict(figures={field: (99.9 % quantile, maximum of max(err - c kappa, 0)
    over the well-conditioned records, number of ill-conditioned ones)}, counts={capped check: violations}, fails=[...], ok=bool)."""
    d = results["_def"]
    n = d["n_paths"] + d["n_nodes"]
    fails = CR.judge(results, n, scenario, report=report, bars=BARS if bars is None else bars)
    counts = {name: int((c.err > 0).sum()) for name, c in results.items() if not name.startswith("_") and c.kappa is None and c.cap}
    return dict(figures=CR.figures(results, C_KAPPA), counts=counts, fails=fails, ok=not fails)


def flagged_share(results_bug, results_ok, field, bars=None):
    """Of the well-conditioned records of `field` whose prediction the seeded mistake moved (the err changed), the share outside the
    field's hard bar; and the number touched."""
    bars = BARS if bars is None else bars
    cb, c0 = results_bug[field], results_ok[field]
    assert np.array_equal(cb.idx, c0.idx)
    touched = cb.err != c0.err
    slack = C_KAPPA * np.maximum(cb.kappa, c0.kappa)
    well = slack <= ILL_KAPPA
    t = touched & well
    out = (cb.err - slack) > bars[field][1]
    return (float(out[t].mean()) if t.any() else 1.0), int(t.sum())


# ---- the claimed densities from first principles (independent of every formula above) ----------------------------------------------
def density_estimate(paths, num_core_total):
    """At padding 2 a thread has one candidate, the next-event sample at its first hit: m = 1 and sample_pdf - fix_pdf is the claimed
    next-event density alone, so sum_threads sum_rgb contri / (sample_pdf - fix_pdf) / threads estimates the image mean of sum_rgb of
    the direct radiance from the area lights (threads without a record count 0).  Returns (estimate, its standard error from its own
    sample variance)."""
    with np.errstate(all="ignore"):
        v = _f64(paths["contri"]).sum(1) / (_f64(paths["sample_pdf"]) - _f64(paths["fix_pdf"]))
    v = np.where(np.isfinite(v), v, 0.0)
    n = float(num_core_total)
    mean = v.sum() / n
    var = (v * v).sum() / n - mean * mean
    return float(mean), float(np.sqrt(max(var, 0.0) / n))


def _ray_hits(O, D, T, tmin, tmax):
    """(t, triangle) of the first crossing of the rays O + t D, t in (tmin, tmax), with the triangles T (brute force, float64)"""
    e1, e2 = T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
    best_t, best_i = np.full(len(O), np.inf), np.full(len(O), -1, np.int64)
    with np.errstate(all="ignore"):
        for j in range(len(T)):
            pv = np.cross(D, e2[j])
            det = _dot(pv, e1[j])
            tv = O - T[j, 0]
            u = _dot(tv, pv) / det
            qv = np.cross(tv, e1[j])
            v = _dot(qv, D) / det
            t = _dot(qv, e2[j]) / det
            hit = (np.abs(det) > 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > tmin) & (t < tmax) & (t < best_t)
            best_t, best_i = np.where(hit, t, best_t), np.where(hit, j, best_i)
    return best_t, best_i


def direct_light_quadrature(scene, camera, n_img, n_light, env=None):
    """The image mean of sum_rgb of the radiance that reaches the camera after ONE reflection of light from the area lights (one-sided
    emitters; a primary ray that misses or meets an emitter counts 0), by the midpoint rule: n_img x n_img camera rays over the image,
    first hit by brute force over all triangles, then n_light x n_light points on every quad light (a barycentric grid of n_light^2
    sub-triangles on every triangle of a mesh light) with brute-force visibility and tests/bsdf_ref's Eval."""
    eye, U, V, Wv = (_f64(x) for x in camera)
    lights = scene_lights(scene, env)
    tris, tri_mat, tri_emit = scene_triangles(scene, lights)
    j = (np.arange(n_img) + 0.5) / n_img
    jx, jy = np.meshgrid(j, j, indexing="ij")
    D = _unit((2 * jx.reshape(-1, 1) - 1) * U + (2 * jy.reshape(-1, 1) - 1) * V + Wv)
    O = np.broadcast_to(eye, D.shape)
    t, ti = _ray_hits(O, D, tris, 1e-3, 1e16)
    live = (ti >= 0) & ~tri_emit[np.clip(ti, 0, len(tris) - 1)]
    P, Dl, tl = (O + t[:, None] * D)[live], D[live], ti[live]
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    tn = _unit(np.cross(e1, e2))
    N = tn[tl]
    N = np.where((_dot(N, Dl) > 0)[:, None], -N, N)
    base_col = np.array([np.asarray(m.get("color", (1, 1, 1)), np.float32) for m in scene.materials]).astype(np.float64)
    M = CR.materials(scene, tri_mat[tl], base_col[tri_mat[tl]])
    pts = []                                        # (position, normal, dA, Le) of every quadrature point on the lights
    for L in lights:
        if L["type"] == 0:
            g = (np.arange(n_light) + 0.5) / n_light
            a, b = np.meshgrid(g, g, indexing="ij")
            Y = L["corner"] + a.reshape(-1, 1) * L["u"] + b.reshape(-1, 1) * L["v"]
            pts.append((Y, np.broadcast_to(L["normal"], Y.shape), np.full(len(Y), L["area"] / len(Y)), _f64(L["emission"])))
        elif L["type"] == 2:
            bc = [((i + (1 + s) / 3.0) / n_light, (jj + (1 + s) / 3.0) / n_light) for i in range(n_light) for jj in range(n_light - i) for s in (0, 1) if s == 0 or jj < n_light - i - 1]
            bc = np.array(bc)
            for T in L["tris"]:
                a1, a2 = T[1] - T[0], T[2] - T[0]
                cr = np.cross(a1, a2)
                Y = T[0] + bc[:, :1] * a1 + bc[:, 1:] * a2
                pts.append((Y, np.broadcast_to(cr / np.linalg.norm(cr), Y.shape), np.full(len(Y), 0.5 * np.linalg.norm(cr) / len(Y)), _f64(L["emission"])))
    total = np.zeros(len(P))
    for Y, NY, dA, Le in pts:
        for q in range(len(Y)):
            vec = Y[q] - P
            r2 = _dot(vec, vec)
            r = np.sqrt(r2)
            c = vec / r[:, None]
            facing = _dot(vec, NY[q]) < 0
            tt, _ = _ray_hits(P, c, tris[~tri_emit], 1e-3, r - 1e-3)
            vis = ~np.isfinite(tt) & facing
            gq = np.abs(_dot(c, N)) * np.abs(_dot(c, NY[q])) / r2
            with np.errstate(all="ignore"):
                f = CR.B.eval(M, N, -Dl, c)
            total += np.where(vis, (f * Le).sum(-1) * gq * dA[q], 0.0)
    return float(total.sum() / len(D))
