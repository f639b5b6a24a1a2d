"""Float64 numpy definition of the Disney BSDF the renderer inherits (OptiXPathTracer/cuProg.h), written from the mathematics and not
from oracle/bsdf.h's operation order, shared by tests/test_bsdf_definition_cpu.py and tests/test_gpu_bsdf_definition.py.

A material is a dict with the scene's keys (color, metallic, roughness, specular, specular_tint, subsurface, sheen, sheen_tint,
clearcoat, clearcoat_gloss; a missing key takes the MaterialData() default); every value may be an array that broadcasts against the
leading axes of the directions.  N, V, L are (..., 3) and are taken as given: nothing but the half vector is normalised.

  half vector            h = (L + V) / |L + V|;  theta_l, theta_v, theta_h from N, theta_d = angle(L, h)
  Schlick weight         w(u) = clamp(1 - u, 0, 1)^5                                                   (cuProg.h:686-691)
  GTR1 (clearcoat)       D1 = (a^2 - 1) / (pi ln a^2 (sin^2 theta_h + a^2 cos^2 theta_h)), 1 / pi at a >= 1   (693-699)
  GTR2 (specular)        D2 = a^2 / (pi (sin^2 theta_h + a^2 cos^2 theta_h)^2), a = max(0.001, roughness)     (701-706, 764)
  Smith GGX              G1(x, g) = 2 x / (x + sqrt(g^2 + x^2 - g^2 x^2)); the source's smithG_GGX is G1 / (2 x)   (708-713)
  Eval (735-799)         zero unless N.L > 0 and N.V > 0; else
                           (1 - metallic) [ C / pi ((1 - subsurface) Fd + subsurface Sub) + w(theta_d) sheen Csheen ]
                           + D2 F G1(N.L, g) G1(N.V, g) / (4 N.L N.V) + clearcoat / 4  D1 Fr G1(N.L, 1/4) G1(N.V, 1/4) / (4 N.L N.V)
                         Fd = (1 + (F90 - 1) w_l)(1 + (F90 - 1) w_v), F90 = 1/2 + 2 roughness cos^2 theta_d
                         Sub = 5/4 (Fss (1 / (N.L + N.V) - 1/2) + 1/2), Fss as Fd with F90 = roughness cos^2 theta_d
                         F = Cspec0 + (1 - Cspec0) w(theta_d), Cspec0 = lerp(0.08 specular lerp(1, tint, specular_tint), C, metallic)
                         tint = C / (0.3 r + 0.6 g + 0.1 b) (1 for black), Csheen = lerp(1, tint, sheen_tint), g = (1/2 + roughness/2)^2
                         Fr = 0.04 + 0.96 w(theta_d), clearcoat a = lerp(0.1, 0.001, clearcoat_gloss)
  Sample (826-866)       three uniforms p, r1, r2; diffuseRatio = (1 - metallic) / 2.  p < diffuseRatio: the cosine lobe, disk radius
                         sqrt(r1) at azimuth 2 pi r2.  Else a half vector at azimuth 2 pi r1, cos^2 theta_h = (1 - r2) /
                         (1 + (a^2 - 1) r2), and V mirrored in it.  Both in the frame of Onb (81-112): binormal (-n.y, n.x, 0) where
                         |n.x| > |n.z|, else (0, -n.z, n.y), normalised; tangent = binormal x normal.
  Pdf (868-899)          diffuseRatio |N.L| / pi + (1 - diffuseRatio) (c D1 (1 - k) + c D2 k) / (4 |L.h|), c = |N.h|, k = 1 / (1 + clearcoat)
  random numbers         lcg: s <- 1664525 s + 1013904223 mod 2^32, the draw is the low 24 bits / 2^24 (cuda/random.h:49-67)

sampled_density is what Sample does, which is NOT Pdf: no clearcoat lobe is ever drawn and the cosine lobe has no mass below the
surface ("the BSDF against its definition")."""
import numpy as np

LCG_A, LCG_C, M32 = 1664525, 1013904223, 1 << 32
LCG_A_INV = pow(LCG_A, -1, M32)
DEFAULTS = dict(color=(1.0, 1.0, 1.0), metallic=0.0, roughness=0.5, specular=0.5, specular_tint=0.0, subsurface=0.0, sheen=0.0,
                sheen_tint=0.5, clearcoat=0.0, clearcoat_gloss=1.0)
KEYS = ("metallic", "roughness", "specular", "specular_tint", "subsurface", "sheen", "sheen_tint", "clearcoat", "clearcoat_gloss")


def _m(mat, key):
    return np.asarray(mat.get(key, DEFAULTS[key]), np.float64)


def _dot(a, b):
    return (a * b).sum(-1)


def _unit(v):
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt(_dot(v, v))[..., None]


def _w5(u):
    return np.clip(1.0 - u, 0.0, 1.0) ** 5


def _mix(a, b, t):
    return a + (b - a) * t


def specular_alpha(mat):
    return np.maximum(0.001, _m(mat, "roughness"))


def clearcoat_alpha(mat):
    return _mix(0.1, 0.001, _m(mat, "clearcoat_gloss"))


def diffuse_ratio(mat):
    return 0.5 * (1.0 - _m(mat, "metallic"))


def gtr1(c, a):
    a2 = a * a
    with np.errstate(divide="ignore", invalid="ignore"):
        d = (a2 - 1.0) / (np.pi * np.log(a2) * ((1.0 - c * c) + a2 * c * c))
    return np.where(a >= 1.0, 1.0 / np.pi, d)


def gtr2(c, a):
    a2 = a * a
    return a2 / (np.pi * ((1.0 - c * c) + a2 * c * c) ** 2)


def _g1(x, g):
    return 2.0 * x / (x + np.sqrt(g * g + x * x - g * g * x * x))


def onb(N):
    """tangent, binormal of cuProg.h:81-112 for normals (..., 3)"""
    N = np.asarray(N, np.float64)
    x, y, z = N[..., 0], N[..., 1], N[..., 2]
    first = np.abs(x) > np.abs(z)
    zero = np.zeros_like(x)
    b = _unit(np.where(first[..., None], np.stack([-y, x, zero], -1), np.stack([zero, -z, y], -1)))
    return np.cross(b, N), b


def eval(mat, N, V, L):   # noqa: A001 (the operation's name)
    N, V, L = (np.asarray(a, np.float64) for a in (N, V, L))
    nl, nv = _dot(N, L), _dot(N, V)
    live = (nl > 0.0) & (nv > 0.0)
    h = _unit(L + V)
    nh, ld = _dot(N, h), _dot(L, h)
    C = np.asarray(mat.get("color", DEFAULTS["color"]), np.float64)
    metallic, rough = _m(mat, "metallic")[..., None], _m(mat, "roughness")
    lum = (0.3 * C[..., 0] + 0.6 * C[..., 1] + 0.1 * C[..., 2])[..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        tint = np.where(lum > 0.0, C / lum, 1.0)
        spec0 = _mix(0.08 * _m(mat, "specular")[..., None] * _mix(1.0, tint, _m(mat, "specular_tint")[..., None]), C, metallic)
        wl, wv, wd = _w5(nl), _w5(nv), _w5(ld)

        def retro(f90):
            return (1.0 + (f90 - 1.0) * wl) * (1.0 + (f90 - 1.0) * wv)
        fd = retro(0.5 + 2.0 * rough * ld * ld)
        sub = 1.25 * (retro(rough * ld * ld) * (1.0 / (nl + nv) - 0.5) + 0.5)
        body = (_mix(fd, sub, _m(mat, "subsurface")) / np.pi)[..., None] * C
        sheen = (wd * _m(mat, "sheen"))[..., None] * _mix(1.0, tint, _m(mat, "sheen_tint")[..., None])
        g = (0.5 + 0.5 * rough) ** 2
        spec = (gtr2(nh, specular_alpha(mat)) * _g1(nl, g) * _g1(nv, g) / (4.0 * nl * nv))[..., None] * (spec0 + (1.0 - spec0) * wd[..., None])
        coat = 0.25 * _m(mat, "clearcoat") * gtr1(nh, clearcoat_alpha(mat)) * (0.04 + 0.96 * wd) * _g1(nl, 0.25) * _g1(nv, 0.25) / (4.0 * nl * nv)
        out = (1.0 - metallic) * (body + sheen) + spec + coat[..., None]
    return np.where(live[..., None], out, 0.0)


def _lobes(mat, N, V, L):
    N, V, L = (np.asarray(a, np.float64) for a in (N, V, L))
    h = _unit(L + V)
    c = np.abs(_dot(N, h))
    with np.errstate(invalid="ignore", divide="ignore"):
        jac = c / (4.0 * np.abs(_dot(L, h)))
    return _dot(N, L), gtr2(c, specular_alpha(mat)) * jac, gtr1(c, clearcoat_alpha(mat)) * jac


def pdf(mat, N, V, L):
    nl, s2, s1 = _lobes(mat, N, V, L)
    k = 1.0 / (1.0 + _m(mat, "clearcoat"))
    dr = diffuse_ratio(mat)
    return dr * np.abs(nl) / np.pi + (1.0 - dr) * (s1 * (1.0 - k) + s2 * k)


def sampled_density(mat, N, V, L):
    """The density of Sample's output per solid angle: the cosine lobe above the surface only, the GTR2 lobe everywhere, no GTR1."""
    nl, s2, _ = _lobes(mat, N, V, L)
    dr = diffuse_ratio(mat)
    return dr * np.maximum(nl, 0.0) / np.pi + (1.0 - dr) * s2


def sample(mat, N, V, p, r1, r2):
    N, V = np.asarray(N, np.float64), np.asarray(V, np.float64)
    p, r1, r2 = (np.asarray(a, np.float64) for a in (p, r1, r2))
    t, b = onb(N)

    def world(x, y, z):
        return x[..., None] * t + y[..., None] * b + z[..., None] * N
    rad, phi = np.sqrt(r1), 2.0 * np.pi * r2
    diffuse = world(rad * np.cos(phi), rad * np.sin(phi), np.sqrt(np.maximum(0.0, 1.0 - r1)))
    a2 = specular_alpha(mat) ** 2
    c2 = (1.0 - r2) / (1.0 + (a2 - 1.0) * r2)
    c, s, phi = np.sqrt(c2), np.sqrt(np.maximum(0.0, 1.0 - c2)), 2.0 * np.pi * r1
    h = world(s * np.cos(phi), s * np.sin(phi), c)
    mirrored = 2.0 * _dot(V, h)[..., None] * h - V
    return np.where((p < diffuse_ratio(mat))[..., None], diffuse, mirrored)


def draws(seed):
    """The three LCG draws of Sample (probability, r1, r2 as 24-bit integers) and the seed afterwards, in integers."""
    s = np.asarray(seed, np.uint64)
    out = []
    for _ in range(3):
        s = (np.uint64(LCG_A) * s + np.uint64(LCG_C)) & np.uint64(M32 - 1)
        out.append(s & np.uint64(0xFFFFFF))
    return out[0], out[1], out[2], s.astype(np.uint32)


def uniforms(seed):
    p, r1, r2, after = draws(seed)
    k = 1.0 / (1 << 24)
    return p * k, r1 * k, r2 * k, after


def seeds_pinning(which, value24):
    """The 256 seeds whose draw number `which` (0 probability, 1 r1, 2 r2) is exactly value24: the state after that draw is value24
    under any upper byte, and the LCG runs backwards through the multiplier's inverse."""
    assert which in (0, 1, 2) and 0 <= int(value24) < (1 << 24)
    out = []
    for hi in range(256):
        s = (hi << 24) | int(value24)
        for _ in range(which + 1):
            s = (LCG_A_INV * (s - LCG_C)) % M32
        out.append(s)
    return np.array(out, np.uint32)


def local(N, L):
    """cos theta and the azimuth in [0, 2 pi) of L in the Onb frame of N."""
    t, b = onb(N)
    L = np.asarray(L, np.float64)
    return _dot(L, N), np.mod(np.arctan2(_dot(L, b), _dot(L, t)), 2.0 * np.pi)


def cell_integrals(fn, N, V, nc, nphi, s):
    """Integrals of fn(L) over the nc x nphi equal-area cells in (cos theta in [0, 1], phi) of the Onb frame of N: the midpoint rule
    on s x s sub-cells per cell.  (V is the caller's; fn closes over it.  Kept in the signature so a cell's meaning is explicit.)"""
    N = np.asarray(N, np.float64)
    t, b = onb(N)
    phi = (np.arange(nphi * s) + 0.5) * (2.0 * np.pi / (nphi * s))
    cp, sp = np.cos(phi), np.sin(phi)
    out = np.zeros((nc, nphi))
    wt = (1.0 / (nc * s)) * (2.0 * np.pi / (nphi * s))
    for i in range(nc):
        c = (i * s + np.arange(s) + 0.5) / (nc * s)
        sn = np.sqrt(1.0 - c * c)
        L = (sn[:, None] * cp[None, :])[..., None] * t + (sn[:, None] * sp[None, :])[..., None] * b + c[:, None, None] * N
        out[i] = fn(L).reshape(s, nphi, s).sum((0, 2)) * wt
    return out


def condition(mat, N, V, L):
    """t2 = 1 + (a^2 - 1)(N.h)^2 of the specular lobe and t1, the same of the clearcoat's a: the two denominators whose cancellation
    governs what FP32 arithmetic of GTR2 / GTR1 can deliver (a relative error of order 2^-24 / t)."""
    N, V, L = (np.asarray(a, np.float64) for a in (N, V, L))
    c2 = _dot(N, _unit(L + V)) ** 2
    return 1.0 + (specular_alpha(mat) ** 2 - 1.0) * c2, 1.0 + (clearcoat_alpha(mat) ** 2 - 1.0) * c2
