"""The float64 all-triangles verdict on ray-casting answers (numpy only; no BVH, no float32 arithmetic of its own).

Every traversal path of the product is compared elsewhere with ANOTHER traversal.  This module judges an answer against the scene's
triangles: for each ray it evaluates every triangle in float64 and decides which answers a correct float32 ray caster may give.

Triangles: the scene's own first, then two per quad light, (c, c+u, (c+u)+(c+v)-c) and (c, that fourth corner, c+v), the corners built
in float32 as the scene set-up does and widened.  Light triangles are single-sided for closest-hit (culled when n.d > 0) and two-sided
for any-hit.  A ray is eight float32 values [o, tmin, d, tmax], widened.

Per ray and triangle: the plane distance t, cos = n^.d^, dist = the in-plane inward distance from the plane point to the nearest edge
line, sin(phi) = |e1 x e2| / (|e1||e2|) (the angle at P0: what Moller-Trumbore's determinant sees).  With eps = 2^-24 and ext the
largest absolute vertex coordinate:
    dw = K eps (ext + max|o| + |t||d|)                                          rounding of the hit point, across the ray
    tt = max(1e-5 max(1,|t|), KT eps (|o-P0| + ext) / (sin(phi) max(|cos|,1e-4) |d|))   rounding of the distance
    clear hit:    dist|cos| > dw, |cos| > 1e-4, (culled: cos < -1e-4), tmin + tt < t < tmax - tt
    possible hit: dist max(|cos|,1e-4) > -dw,   (culled: cos < 1e-4),  tmin - tt < t < tmax + tt
Closest-hit answer (tri, t_dev): tri == -1 is accepted iff no clear hit exists; a triangle iff it is a possible hit,
|t_dev - t_tri| <= tt, and t_tri is not beyond the nearest clear hit by more than 1e-5 max(1, t).  Any-hit answer: 0 (occluded) is
accepted iff some possible hit exists (no culling), 1 (visible) iff no clear hit exists.
A ray is AMBIGUOUS when more than one answer is acceptable -- a property of ray and verdict, never of the device.  A ray with a
possible hit at |cos| <= 1e-4 (a coplanar ray) has no defined answer: it is reported as ambiguous and is never counted as passed.
A ZERO-AREA triangle (|e1 x e2| = 0 in float64: two equal corners, three collinear ones) is never a hit: neither clear nor possible nor
coplanar, set explicitly and not left to NaN compares; an answer that names one is unexplained.  Bit-identical copies of one triangle
are ONE answer: they count once among the acceptable answers of a ray, and the "second-nearest clear hit" is the nearest of OTHER
geometry (a scene without copies sees no difference).

K and KT start at 64 and 16: tests/test_ray_verdict_cpu.py holds these constants to the CPU oracle (zero unexplained answers) and to
seeded corruptions of its answers (all flagged).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

EPS = 2.0 ** -24
K = 64.0
KT = 16.0
COS_MIN = 1e-4
T_REL = 1e-5


def scene_triangles(scene):
    """(P float64 (T, 3, 3), culled bool (T,), vertex ids int (T, 3)): the scene's triangles, then two per quad light; the ids of light
    corners continue after the scene's vertices."""
    V = np.asarray(scene.vertices, dtype=np.float32)
    I = np.asarray(scene.indices, dtype=np.int64)
    P = [V[I]]
    ids = [I]
    nv = len(V)
    for L in scene.lights:
        c = np.asarray(L["position"], dtype=np.float32)
        a = c + np.asarray(L["u"], dtype=np.float32)
        b = c + np.asarray(L["v"], dtype=np.float32)
        d = (a + b) - c   # float32 throughout
        P.append(np.stack([np.stack([c, a, d]), np.stack([c, d, b])]))
        ids.append(np.array([[nv, nv + 1, nv + 3], [nv, nv + 3, nv + 2]], dtype=np.int64))
        nv += 4
    P = np.concatenate(P).astype(np.float64)
    culled = np.zeros(len(P), dtype=bool)
    culled[len(I):] = True
    return P, culled, np.concatenate(ids)


class Verdict:
    def __init__(self, P, culled, k=K, kt=KT):
        self.P = np.asarray(P, dtype=np.float64)
        self.culled = np.asarray(culled, dtype=bool)
        self.k, self.kt = float(k), float(kt)
        self.T = len(self.P)
        self.ext = float(np.abs(self.P).max())
        P0, P1, P2 = self.P[:, 0], self.P[:, 1], self.P[:, 2]
        e1, e2 = P1 - P0, P2 - P0
        n = np.cross(e1, e2)
        with np.errstate(invalid="ignore", divide="ignore"):
            nl = np.linalg.norm(n, axis=1)
            self.nhat = n / nl[:, None]
            self.sinphi = nl / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))
            # inward unit normals of the three edge lines, in the triangle's plane: n^ x (B - A) / |B - A|
            self.edge_a = np.stack([P0, P1, P2], 1)
            ed = np.stack([P1 - P0, P2 - P1, P0 - P2], 1)
            ed = ed / np.linalg.norm(ed, axis=2)[..., None]
            self.edge_m = np.cross(self.nhat[:, None, :], ed)
        self.degenerate = ~(nl > 0.0)
        first = {}
        self.group = np.array([first.setdefault(tri.tobytes(), i) for i, tri in enumerate(self.P)], dtype=np.int64)   # first bit-identical copy
        self._copies = bool((self.group != np.arange(self.T)).any())
        self.P0 = P0
        self._nP0 = (self.nhat * P0).sum(1)
        self._mA = (self.edge_m * self.edge_a).sum(2)
        self._P0sq = (P0 * P0).sum(1)

    # ---- the per (ray, triangle) quantities; `sel` picks triangles: None = all (result (B, T)), or an index per ray (result (B, 1))
    def _pairs(self, rays, sel=None):
        r = np.asarray(rays, dtype=np.float32).reshape(-1, 8).astype(np.float64)
        o, d = r[:, None, 0:3], r[:, None, 4:7]
        if sel is None:
            pick = lambda a: a[None]
        else:
            s = np.asarray(sel, dtype=np.int64)
            pick = lambda a: a[s][:, None]
        nhat, P0, sinphi, A, M, culled = pick(self.nhat), pick(self.P0), pick(self.sinphi), pick(self.edge_a), pick(self.edge_m), pick(self.culled)
        degenerate = pick(self.degenerate)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            dl = np.linalg.norm(d, axis=2)                     # (B, 1)
            if sel is None:
                # every triangle: the dot products as matrix products (n^.(P0 - o) = n^.P0 - o.n^, and so on)
                o2, d2 = o[:, 0], d[:, 0]
                h = self._nP0[None] - o2 @ self.nhat.T
                dn = d2 @ self.nhat.T
                t = h / dn
                dist = None
                for k in range(3):
                    dk = (o2 @ self.edge_m[:, k].T - self._mA[None, :, k]) + t * (d2 @ self.edge_m[:, k].T)
                    dist = dk if dist is None else np.minimum(dist, dk)
                oP0 = np.sqrt(np.maximum((o2 * o2).sum(1)[:, None] + self._P0sq[None] - 2.0 * (o2 @ self.P0.T), 0.0))
            else:
                h = ((P0 - o) * nhat).sum(2)                   # n^.(P0 - o)
                dn = (d * nhat).sum(2)
                t = h / dn
                dist = None
                for k in range(3):
                    dk = ((o - A[:, :, k]) * M[:, :, k]).sum(2) + t * (d * M[:, :, k]).sum(2)
                    dist = dk if dist is None else np.minimum(dist, dk)
                oP0 = np.linalg.norm(o - P0, axis=2)
            cos = dn / dl
            omax = np.abs(o).max(2)
            dw = self.k * EPS * (self.ext + omax + np.abs(t) * dl)
            dw0 = self.k * EPS * (self.ext + omax)
            ac = np.abs(cos)
            acm = np.maximum(ac, COS_MIN)
            tt = np.maximum(T_REL * np.maximum(1.0, np.abs(t)), self.kt * EPS * (oP0 + self.ext) / (sinphi * acm * dl))
        return dict(t=t, cos=cos, ac=ac, acm=acm, dist=dist, dw=dw, dw0=dw0, tt=tt, h=h, culled=culled, degenerate=degenerate)

    @staticmethod
    def _flags(q, tmin, tmax, cull):
        """clear / possible / coplanar of every pair over the interval (tmin, tmax) (each (B, 1)); cull: emitters are single-sided."""
        with np.errstate(invalid="ignore", over="ignore"):
            t, tt, cos = q["t"], q["tt"], q["cos"]
            clear = (q["dist"] * q["ac"] > q["dw"]) & (q["ac"] > COS_MIN) & (t > tmin + tt) & (t < tmax - tt)
            geom = q["dist"] * q["acm"] > -q["dw"]
            rng = (t > tmin - tt) & (t < tmax + tt)
            possible = geom & rng
            # a ray (nearly) in the plane of a triangle it comes near: no defined answer.  (cos == 0 leaves t infinite or undefined: a ray
            # that lies within rounding of the plane itself is counted as near, whatever the triangle's extent)
            coplanar = (q["ac"] <= COS_MIN) & (possible | (np.abs(q["h"]) <= q["dw0"]))
            if cull:
                clear &= ~q["culled"] | (cos < -COS_MIN)
                possible &= ~q["culled"] | (cos < COS_MIN)
            solid = ~q["degenerate"]   # a zero-area triangle is never a hit
            clear, possible, coplanar = clear & solid, possible & solid, coplanar & solid
        return clear, possible, coplanar

    def _summary(self, q, tmin, tmax, cull):
        clear, possible, coplanar = self._flags(q, tmin, tmax, cull)
        B = clear.shape[0]
        rows = np.arange(B)
        tc = np.where(clear, q["t"], np.inf)
        i1 = tc.argmin(1)
        t1 = tc[rows, i1]
        has = np.isfinite(t1)
        if self._copies:
            tc[self.group[None, :] == self.group[i1][:, None]] = np.inf   # the nearest and its bit-identical copies
        else:
            tc[rows, i1] = np.inf
        i2 = tc.argmin(1)
        t2 = tc[rows, i2]
        lim = np.where(has, t1 + T_REL * np.maximum(1.0, np.abs(t1)), np.inf)
        with np.errstate(invalid="ignore"):
            acc = possible & (q["t"] <= lim[:, None])
        if self._copies:   # copies of one triangle are one answer
            ug, inv = np.unique(self.group, return_inverse=True)
            onehot = np.zeros((self.T, len(ug)), dtype=np.float32)
            onehot[np.arange(self.T), inv] = 1.0
            n_acc = ((acc.astype(np.float32) @ onehot) > 0).sum(1) + (~has)
        else:
            n_acc = acc.sum(1) + (~has)
        with np.errstate(invalid="ignore", divide="ignore"):
            margin = np.where(has, (q["dist"] * q["ac"] / q["dw"])[rows, i1], np.inf)
        cop = coplanar.any(1)
        return dict(has_clear=has, t1=t1, tri1=np.where(has, i1, -1), t2=t2, tri2=np.where(np.isfinite(t2), i2, -1), lim=lim, n_acc=n_acc,
                    has_possible=possible.any(1), coplanar=cop, margin=margin,
                    ambiguous=(n_acc > 1) | cop,                       # closest-hit: more than one acceptable answer
                    ambiguous_any=(possible.any(1) & ~has) | cop)      # any-hit: both 0 and 1 acceptable

    def table(self, rays, tmax_any=None, block=128):
        """The per-ray summaries of the brute force, computed once per ray set: "closest" over the rays' own interval (emitters culled),
        "open" the same with tmax = 1e16 (the pooled pass's own rays), "any" over (tmin, tmax_any) without culling (default: the rays' tmax)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = len(rays)
        tmin = rays[:, 3].astype(np.float64)
        tmax = rays[:, 7].astype(np.float64)
        ta = tmax if tmax_any is None else np.asarray(tmax_any, dtype=np.float32).astype(np.float64)
        same_open = bool((rays[:, 7] == np.float32(1e16)).all())
        parts = {"closest": [], "any": [], "open": []}
        def one(b):
            sl = slice(b, min(n, b + block))
            q = self._pairs(rays[sl])
            c = self._summary(q, tmin[sl, None], tmax[sl, None], True)
            a = self._summary(q, tmin[sl, None], ta[sl, None], False)
            op = None if same_open else self._summary(q, tmin[sl, None], np.full((sl.stop - sl.start, 1), float(np.float32(1e16))), True)
            return c, a, op
        with ThreadPoolExecutor(max_workers=4) as ex:   # (numpy releases the interpreter lock inside its loops)
            for c, a, op in ex.map(one, range(0, n, block)):
                parts["closest"].append(c); parts["any"].append(a)
                if op is not None: parts["open"].append(op)
        out = {"rays": rays, "tmax_any": ta.astype(np.float32)}
        for name, lst in parts.items():
            if lst:
                out[name] = {key: np.concatenate([p[key] for p in lst]) for key in lst[0]}
        if same_open:
            out["open"] = out["closest"]
        return out

    # ---- judging answers ---------------------------------------------------------------------------------------------------------
    def judge_closest(self, tab, tri, t, which="closest", sel=None):
        """Judges closest-hit answers (tri, t) on rays tab["rays"][sel] against summary `which` ("closest" or "open").  Returns a dict:
        ok (the answer is acceptable), unexplained (= ~ok on a ray that has a defined answer), ambiguous, dt_over_tt (nan on misses),
        margin (dist|cos| / dw of the nearest clear hit)."""
        sel = np.arange(len(tab["rays"])) if sel is None else np.asarray(sel)
        S = {k: v[sel] for k, v in tab[which].items()}
        rays = tab["rays"][sel].copy()
        if which == "open":
            rays[:, 7] = np.float32(1e16)
        tri = np.asarray(tri, dtype=np.int64)
        t = np.asarray(t, dtype=np.float32).astype(np.float64)
        hit = tri >= 0
        valid = hit & (tri < self.T)
        ok = np.where(hit, False, ~S["has_clear"])
        ratio = np.full(len(sel), np.nan)
        if valid.any():
            idx = np.nonzero(valid)[0]
            q = self._pairs(rays[idx], tri[idx])
            _, possible, _ = self._flags(q, rays[idx, 3:4].astype(np.float64), rays[idx, 7:8].astype(np.float64), True)
            with np.errstate(invalid="ignore", divide="ignore"):
                dt = np.abs(t[idx] - q["t"][:, 0])
                r = dt / q["tt"][:, 0]
                good = possible[:, 0] & (dt <= q["tt"][:, 0]) & (q["t"][:, 0] <= S["lim"][idx])
            ok[idx] = good
            ratio[idx] = r
        return dict(ok=ok, unexplained=~ok & ~S["coplanar"], ambiguous=S["ambiguous"], dt_over_tt=ratio, margin=S["margin"])

    def pair(self, rays, tri):
        """(t, tt, dist|cos| / dw) of ray i against triangle tri[i], in float64"""
        q = self._pairs(rays, tri)
        with np.errstate(invalid="ignore", divide="ignore"):
            return q["t"][:, 0], q["tt"][:, 0], (q["dist"] * q["ac"] / q["dw"])[:, 0]

    def judge_any(self, tab, vis, sel=None):
        sel = np.arange(len(tab["rays"])) if sel is None else np.asarray(sel)
        S = {k: v[sel] for k, v in tab["any"].items()}
        vis = np.asarray(vis)
        ok = np.where(vis == 0, S["has_possible"], ~S["has_clear"]) & ((vis == 0) | (vis == 1))
        return dict(ok=ok, unexplained=~ok & ~S["coplanar"], ambiguous=S["ambiguous_any"])


def report(j):
    """(ambiguous share, worst |dt| / tt over the unambiguous hits, smallest clear margin over the unambiguous rays)"""
    un = ~j["ambiguous"]
    with np.errstate(invalid="ignore"):
        r = j.get("dt_over_tt")
        worst = float(np.nanmax(np.where(un, r, np.nan))) if r is not None and np.isfinite(np.where(un, r, np.nan)).any() else 0.0
        m = j.get("margin")
        mm = float(np.min(np.where(un & np.isfinite(m), m, np.inf))) if m is not None else float("inf")
    return float(j["ambiguous"].mean()), worst, mm
