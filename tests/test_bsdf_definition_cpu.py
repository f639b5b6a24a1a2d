"""The Disney BSDF against a float64 definition of its own (tests/bsdf_ref.py), on the CPU: the definition's Sample is distributed as
its density says (chi^2), the test notices seeded corruptions, the properties the inherited formulas have are pinned, and the
FP32 oracle (oracle/bsdf.h) is held to the definition, all lobes on, at the inputs where such code goes wrong.
tests/test_gpu_bsdf_definition.py holds the device code to the same definition with the same record families and the same bound.

chi^2: 1 000 000 seeds through the integer LCG and Sample, binned in 12 x 24 equal-area cells of the upper hemisphere around N plus one
bin for everything below the surface; expected counts from the midpoint quadrature of the density (sub-cells doubled until no cell
moves by 1e-3 of the largest); cells expecting fewer than 10 merged; tail probability above 1e-6, the suite's convention.

The bound of the pointwise comparison (d), per record and output (Eval, Pdf, sampled direction):

    |FP32 - float64| <= 2^-24 (C0 + C2 / t2 + C1 / t1 [clearcoat != 0]) scale

t2 = 1 + (a^2 - 1)(N.h)^2 and t1, the same of the clearcoat's a (bsdf_ref.condition): FP32 leaves 1 / t of its digits in the GTR
denominators.  What the oracle showed the form to need, each a property of FP32 arithmetic of the inherited formulas:
  * Eval's scale is its largest component -- or, where that is larger (a black metal: F is the Schlick weight alone), what the
    absolute 2^-24 of L.h moves the specular lobe by, 5 (1 - L.h)^4 D2 G.
  * Pdf's scale is Pdf with its cosine factors at 1 and the GTR1 term at full weight.  |N.h| and |N.L| are dot products of unit
    vectors and carry an absolute 2^-24; and lerp(g1, g2, k) = g1 + (g2 - g1) k passes GTR1 through FP32 even at clearcoat = 0
    (k = 1), which leaves 2^-24 g1 in a Pdf that may be far smaller: 0.4 % of a Pdf of 5e-8 away from the lobe of a 0.0005-rough metal.
  * The sampled direction has no GTR denominator of its own; in its place stand the sampler's two cancelling quantities: t2 :=
    (1 + (a^2 - 1) r2) sin theta_h for the specular lobe (the denominator of cos^2 theta_h, and sinTheta = sqrt(1 - cos^2)),
    sqrt(1 - r1) for the cosine lobe (p.z = sqrt(1 - x^2 - y^2)); no clearcoat term, Sample draws none.  At a = 0.001 the direction
    is off by up to 2.4e-3 (r2 = 1 - 2^-24) and by 4e-4 on random seeds.
The constants are measured from the ORACLE, here (test_oracle_against_the_definition prints the fit and asserts that it rounds to
them): C0 puts the worst record with t2 >= 1/2 and no clearcoat at half the bound, then C2 the worst of all records without clearcoat,
then C1 the worst with clearcoat; each rounded up to one significant digit:

    fitted 36.4, 40.9, 9.4  ->  C0 = 40    C2 = 50    C1 = 10

The oracle's error in units of 2^-24 scale, quantiles 50 / 99 / 100 % per family (worst of direction, Eval, Pdf), as measured:
    random                               3.26 / 2.2e+03 / 2.55e+04      axis normals                3.18 / 3.19e+03 / 2.79e+06
    peak                                 1.53e+03 / 4.68e+06 / 1.83e+07 grazing                     3.5 / 2.65e+03 / 4.52e+03
    retro                                6.63 / 1.47e+06 / 1.3e+07      black / saturated           5.62 / 3.02e+03 / 4.51e+03
    ratio edges                          5.28 / 2.9e+03 / 2.38e+04      pinned r2 = 0               1.63 / 1.81 / 1.81
    pinned r2 = 2^24 - 1                 2.88 / 3.97e+04 / 3.97e+04     pinned r1 = 0               3.45 / 852 / 852
    pinned r1 = 2^24 - 1                 2.94 / 1.88e+03 / 1.88e+03     pinned probability = diffuseRatio          3.07 / 1.86e+03 / 1.86e+03
    pinned probability = diffuseRatio - 2^-24   1.75 / 2.18 / 2.18
(1.83e+07 is a relative error of 1.09: at the clamp a = 0.001, t2 = 1.1e-6 from the peak, FP32 GTR2 keeps no digit; the large figures
of the other families are records of a = 0.001 too.  Where t2 >= 0.05 and clearcoat = 0 every Eval and Pdf is within 1e-5, asserted.)
"""
import math

import numpy as np
import pytest

from tests import bsdf_ref as B
from tests.test_gpu_mesh_light import _chi2_sf

EPS32 = 2.0 ** -24
C0, C2, C1 = 40.0, 50.0, 10.0        # measured from the oracle: see the module docstring

NC, NPHI, NSAMPLES = 12, 24, 1_000_000
N_AXIS = np.array([0.0, 1.0, 0.0])
N_TILT = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])


def view(N, theta, phi=0.7):
    t, b = B.onb(N)
    return math.sin(theta) * (math.cos(phi) * t + math.sin(phi) * b) + math.cos(theta) * N


def _configs():
    out = []
    for k, (metallic, rough) in enumerate((m, r) for m in (0.0, 0.5, 1.0) for r in (0.1, 0.3, 0.6, 1.0)):
        N = N_AXIS if k % 2 == 0 else N_TILT
        theta = (0.0, 0.8, 1.45)[k % 3]
        out.append(dict(name=f"metallic {metallic:g} roughness {rough:g} N {'+y' if k % 2 == 0 else 'tilted'} view {theta:g} rad",
                        mat=dict(metallic=metallic, roughness=rough), N=N, V=view(N, theta)))
    return out


CONFIGS = _configs()


def chi2_tail(x, df):
    """_chi2_sf, kept inside the range where its closed form neither overflows nor underflows: beyond x = 1400 the tail of any
    df <= 300 is below 1e-150 and reported as 0."""
    assert 0 < df <= 300
    return _chi2_sf(x, df) if x <= 1400.0 else 0.0


def pearson(counts, expected, least=10.0):
    """chi^2 and degrees of freedom after merging, in order of expectation, the cells that expect fewer than `least`."""
    order = np.argsort(expected, kind="stable")
    c, e = counts[order].astype(np.float64), expected[order].astype(np.float64)
    cc, ee, ac, ae = [], [], 0.0, 0.0
    for a, b in zip(c, e):
        ac += a; ae += b
        if ae >= least:
            cc.append(ac); ee.append(ae); ac = ae = 0.0
    if ae > 0 or ac > 0:
        cc[-1] += ac; ee[-1] += ae
    cc, ee = np.array(cc), np.array(ee)
    return float(((cc - ee) ** 2 / ee).sum()), len(cc) - 1


_CELLS = {}


def expected_cells(density, mat, N, V, s_max=256, tol=1e-3):
    """Converged cell integrals of `density` (NC x NPHI) and the relative change of the last doubling; cached per configuration."""
    key = (density.__name__, tuple(sorted((k, float(v)) for k, v in mat.items())), tuple(N), tuple(V), s_max)
    if key not in _CELLS:
        def fn(L):
            return density(mat, N, V, L)
        s, prev = 16, B.cell_integrals(fn, N, V, NC, NPHI, 16)
        while True:
            s *= 2
            cur = B.cell_integrals(fn, N, V, NC, NPHI, s)
            change = float(np.abs(cur - prev).max() / cur.max())
            prev = cur
            if change <= tol or s >= s_max:
                break
        _CELLS[key] = (cur, change, s)
    return _CELLS[key]


def bin_directions(N, L):
    """Counts per cell (NC * NPHI) with the below-surface count appended."""
    c, phi = B.local(N, L)
    up = c > 0.0
    i = np.minimum((c[up] * NC).astype(np.int64), NC - 1)
    j = np.minimum((phi[up] * (NPHI / (2.0 * np.pi))).astype(np.int64), NPHI - 1)
    return np.append(np.bincount(i * NPHI + j, minlength=NC * NPHI), int((~up).sum()))


def chi2_of(counts, cells):
    n = counts.sum()
    expected = np.append(cells.ravel(), max(0.0, 1.0 - cells.sum())) * n
    x, df = pearson(counts, expected)
    return x, df, chi2_tail(x, df)


def draw_uniforms(cfg_index, n=NSAMPLES):
    seeds = np.random.default_rng(1000 + cfg_index).integers(0, 2 ** 32, n, dtype=np.uint64)
    return seeds, B.uniforms(seeds)


def sampled_counts(cfg_index, cfg, transform=None, mat=None, mirror=False):
    _, (p, r1, r2, _) = draw_uniforms(cfg_index)
    m = cfg["mat"] if mat is None else mat
    if transform is not None:
        p, r1, r2 = transform(m, p, r1, r2)
    L = B.sample(m, cfg["N"], cfg["V"], p, r1, r2)
    if mirror:                            # the sampled direction's azimuth mirrored about the bitangent: its tangent component negated
        t, _ = B.onb(cfg["N"])
        L = L - 2.0 * (L @ t)[:, None] * t
    return bin_directions(cfg["N"], L)


# ------------------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("k", range(len(CONFIGS)))
def test_sample_is_distributed_as_pdf(k):
    cfg = CONFIGS[k]
    cells, change, s = expected_cells(B.pdf, cfg["mat"], cfg["N"], cfg["V"])
    assert change <= 1e-3, (change, s)
    x, df, p = chi2_of(sampled_counts(k, cfg), cells)
    print(f"{cfg['name']}: chi^2 = {x:.1f} with {df} degrees of freedom, tail probability {p:.3g} ({s} x {s} sub-cells, last change {change:.1e}, "
          f"mass below the surface {1 - cells.sum():.4f})")
    assert p > 1e-6, (x, df)


# ------------------------------------------------------------------------------------------------------------------ (b)
def _scaled_ratio(m, p, r1, r2):          # diffuseRatio * 0.96: the branch is taken for p < 0.96 diffuseRatio
    return p / 0.96, r1, r2


def _swapped(m, p, r1, r2):               # r1 <-> r2 in the specular lobe: both are uniform, the density is the same
    d = p < B.diffuse_ratio(m)
    return p, np.where(d, r1, r2), np.where(d, r2, r1)


CORRUPTIONS = [("diffuseRatio x 0.96", 1, _scaled_ratio, None), ("roughness x 1.03", 9, None, 1.03), ("azimuth mirrored", 5, None, None)]


@pytest.mark.parametrize("name,k,transform,rough_scale", CORRUPTIONS, ids=[c[0] for c in CORRUPTIONS])
def test_a_corrupted_sampler_is_rejected(name, k, transform, rough_scale):
    cfg = CONFIGS[k]
    cells, _, _ = expected_cells(B.pdf, cfg["mat"], cfg["N"], cfg["V"])
    mat = dict(cfg["mat"], roughness=cfg["mat"]["roughness"] * rough_scale) if rough_scale else None
    x, df, p = chi2_of(sampled_counts(k, cfg, transform, mat, mirror=name == "azimuth mirrored"), cells)
    print(f"{name} in '{cfg['name']}': chi^2 = {x:.1f} with {df} degrees of freedom, tail probability {p:.3g}")
    assert p < 1e-6, (x, df)


def test_swapping_the_specular_uniforms_is_invisible_to_chi2():
    """r1 <-> r2 in the specular lobe draws from the same density (both are uniform), so the chi^2 must NOT reject it: what catches
    such a swap is the pointwise comparison of the sampled direction with the definition's, record by record, in
    test_oracle_against_the_definition and in tests/test_gpu_bsdf_definition.py."""
    k = 5
    cfg = CONFIGS[k]
    cells, _, _ = expected_cells(B.pdf, cfg["mat"], cfg["N"], cfg["V"])
    x, df, p = chi2_of(sampled_counts(k, cfg, _swapped), cells)
    print(f"r1 <-> r2 in '{cfg['name']}': chi^2 = {x:.1f} with {df} degrees of freedom, tail probability {p:.3g}")
    assert p > 1e-6
    _, (pp, r1, r2, _) = draw_uniforms(k, 1000)
    a = B.sample(cfg["mat"], cfg["N"], cfg["V"], pp, r1, r2)
    b = B.sample(cfg["mat"], cfg["N"], cfg["V"], *_swapped(cfg["mat"], pp, r1, r2))
    spec = pp >= B.diffuse_ratio(cfg["mat"])
    assert np.abs(a - b).max(-1)[spec].min() > 1e-4          # ... where every specular record is far outside any FP32 bound


# ------------------------------------------------------------------------------------------------------------------ (c)
COATS = [(0.5, 0.0), (0.5, 1.0), (1.0, 0.0), (1.0, 1.0)]


@pytest.mark.parametrize("coat,gloss", COATS)
def test_pdf_claims_a_clearcoat_lobe_that_sample_never_draws(coat, gloss):
    """Inherited: Pdf mixes GTR1 in with weight 1 - 1 / (1 + clearcoat), Sample draws GTR2 only.  The samples follow sampled_density
    and not Pdf.  (At gloss 1 the GTR1 peak, 1e-3 rad wide, is below the quadrature's resolution: Pdf's cells are then taken at
    64 x 64 sub-cells as they are -- a third to a half of the specular mass is claimed elsewhere and the verdict does not hang on it.)"""
    k = 5
    cfg = CONFIGS[k]
    mat = dict(cfg["mat"], clearcoat=coat, clearcoat_gloss=gloss)
    counts = sampled_counts(k, cfg, mat=mat)
    cells, change, s = expected_cells(B.sampled_density, mat, cfg["N"], cfg["V"])
    assert change <= 1e-3
    x, df, p = chi2_of(counts, cells)
    wrong, _, _ = expected_cells(B.pdf, mat, cfg["N"], cfg["V"], s_max=64)
    xw, dfw, pw = chi2_of(counts, wrong)
    print(f"clearcoat {coat:g} gloss {gloss:g}: against sampled_density chi^2 = {x:.1f} / {df} (tail {p:.3g}); against Pdf chi^2 = {xw:.0f} / {dfw} (tail {pw:.3g})")
    assert p > 1e-6 and pw < 1e-6


def _radial(fn, N, n=400_000):
    """2 pi int_0^{pi/2} fn(L(theta)) sin theta d theta for an integrand symmetric about N: midpoints in ln theta from 1e-8 rad."""
    t, _ = B.onb(N)
    u0, u1 = math.log(1e-8), math.log(0.5 * math.pi)
    th = np.exp(u0 + (np.arange(n) + 0.5) * ((u1 - u0) / n))
    L = np.sin(th)[:, None] * t + np.cos(th)[:, None] * N
    return float((fn(L) * np.sin(th) * th).sum() * ((u1 - u0) / n) * 2.0 * np.pi)


def upper_mass_gtr2(a):
    """V = N: L is above the surface for cos^2 theta_h > 1/2; the sampler's CDF there, r2 = sin^2 / (sin^2 + a^2 cos^2), is 1 / (1 + a^2)."""
    return 1.0 / (1.0 + a * a)


def upper_mass_gtr1(a):
    return 1.0 - math.log(0.5 * (1.0 + a * a)) / math.log(a * a) if a < 1.0 else 0.5


@pytest.mark.parametrize("coat,gloss", COATS)
def test_the_gap_between_pdf_and_density_has_its_closed_form(coat, gloss):
    """At V = N: int_upper (Pdf - sampled_density) = specularRatio (1 - 1 / (1 + clearcoat)) (U1 - U2), U the upper-hemisphere masses of
    the two GTR lobes in closed form."""
    for N in (N_AXIS, N_TILT):
        for metallic, rough in ((0.0, 0.3), (0.5, 0.1), (1.0, 0.6)):
            mat = dict(metallic=metallic, roughness=rough, clearcoat=coat, clearcoat_gloss=gloss)
            got = _radial(lambda L: B.pdf(mat, N, N, L) - B.sampled_density(mat, N, N, L), N)
            a1, a2 = float(B.clearcoat_alpha(mat)), float(B.specular_alpha(mat))
            want = (1.0 - float(B.diffuse_ratio(mat))) * (1.0 - 1.0 / (1.0 + coat)) * (upper_mass_gtr1(a1) - upper_mass_gtr2(a2))
            print(f"clearcoat {coat:g} gloss {gloss:g} metallic {metallic:g} roughness {rough:g}: gap {got:+.7f}, closed form {want:+.7f}")
            assert abs(got - want) <= 1e-6, (got, want)


def _random_geometry(rng, n):
    N = B._unit(rng.normal(size=(n, 3)))
    V = B._unit(N + 0.9 * B._unit(rng.normal(size=(n, 3))))
    L = B._unit(rng.normal(size=(n, 3)))
    return N, V, L


def _random_lobes(rng, n, clearcoat=True):
    u = rng.uniform(0.0, 1.0, (n, 8))
    return dict(color=rng.uniform(0.02, 1.0, (n, 3)), metallic=rng.choice([0.0, 1.0, 0.5, 0.3], n), roughness=rng.choice([0.05, 0.1, 0.3, 0.5, 0.8, 1.0, 0.0005], n),
                specular=u[:, 0], specular_tint=u[:, 1], subsurface=u[:, 2], sheen=u[:, 3], sheen_tint=u[:, 4],
                clearcoat=u[:, 5] if clearcoat else np.zeros(n), clearcoat_gloss=u[:, 6])


def test_pdf_is_the_density_without_clearcoat_except_below_the_surface():
    """clearcoat = 0: Pdf == sampled_density above the surface; below it Pdf keeps the cosine lobe's |N.L| / pi, which Sample never
    draws there (inherited: pdfDiff uses |n.L| on both hemispheres)."""
    rng = np.random.default_rng(21)
    n = 20000
    N, V, L = _random_geometry(rng, n)
    mat = _random_lobes(rng, n, clearcoat=False)
    p, d, nl = B.pdf(mat, N, V, L), B.sampled_density(mat, N, V, L), (N * L).sum(-1)
    up = nl > 0
    assert up.sum() > 5000 and (~up).sum() > 5000
    assert np.abs(p[up] - d[up]).max() <= 1e-15 * np.abs(p[up]).max() and (np.abs(p[up] - d[up]) <= 1e-13 * p[up]).all()
    want = B.diffuse_ratio(mat)[~up] * np.abs(nl[~up]) / np.pi
    assert (np.abs((p - d)[~up] - want) <= 1e-13 * p[~up]).all()


BELOW_ROUGHNESS = (0.05, 0.1, 0.2, 0.3, 0.5, 0.7, 0.85, 1.0)


def test_specular_samples_below_the_surface():
    """Inherited: the specular lobe mirrors V in a half vector of the upper hemisphere, which can put L below the surface.  At V = N
    the share is a^2 / (1 + a^2) of the specular samples, smooth in the roughness, 1/2 at roughness 1 (measured with 1e6 seeds,
    metallic 1, beside the closed form):
        roughness   0.05     0.1      0.2      0.3      0.5      0.7      0.85     1.0
        a^2/(1+a^2) 0.00249  0.00990  0.03846  0.08257  0.20000  0.32886  0.41945  0.50000
    At grazing view it is larger still (the chi^2 configurations at 1.45 rad print theirs).  The walks drop such a sample: see DESIGN.md."""
    seeds = np.random.default_rng(22).integers(0, 2 ** 32, NSAMPLES, dtype=np.uint64)
    p, r1, r2, _ = B.uniforms(seeds)
    row, prev = [], 0.0
    for metallic in (1.0, 0.0):
        for rough in BELOW_ROUGHNESS:
            mat = dict(metallic=metallic, roughness=rough)
            for N in (N_AXIS, N_TILT):
                L = B.sample(mat, N, N, p, r1, r2)
                got = float(((L * N).sum(-1) <= 0).mean())
                want = (1.0 - float(B.diffuse_ratio(mat))) * (1.0 - upper_mass_gtr2(rough))
                assert abs(got - want) <= 5.0 * math.sqrt(want * (1 - want) / NSAMPLES), (metallic, rough, got, want)
            if metallic == 1.0:
                row.append((rough, got, want))
                assert want > prev
                prev = want
    print("below-surface share of Sample at V = N, metallic 1 (roughness: measured / closed form): " + "  ".join(f"{r:g}: {g:.5f} / {w:.5f}" for r, g, w in row))
    assert abs(row[-1][2] - 0.5) < 1e-15


def test_eval_is_reciprocal():
    rng = np.random.default_rng(23)
    n = 10000
    N = B._unit(rng.normal(size=(n, 3)))
    V = B._unit(N * rng.uniform(0.05, 1.0, (n, 1)) + B._unit(rng.normal(size=(n, 3))))
    L = B._unit(N * rng.uniform(0.05, 1.0, (n, 1)) + B._unit(rng.normal(size=(n, 3))))
    mat = _random_lobes(rng, n)
    a, b = B.eval(mat, N, V, L), B.eval(mat, N, L, V)
    assert ((a > 0).all(-1)).sum() > 5000
    assert (np.abs(a - b).max(-1) <= 1e-13 * np.abs(a).max(-1)).all()


# ------------------------------------------------------------------------------------------------------------------ (d)
def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def records(mat, N, V, L, seeds=None):
    """(n, 24) uint32 records of the BSDF unit op: material 0-11, N 12-14, V 15-17, L 18-20, seed 21."""
    n = max(len(np.atleast_2d(a)) for a in (N, V, L))
    rec = np.zeros((n, 24), np.float32)
    rec[:, 0:3] = np.asarray(mat.get("color", B.DEFAULTS["color"]))
    for c, key in enumerate(B.KEYS):
        rec[:, 3 + c] = np.asarray(mat.get(key, B.DEFAULTS[key]))
    rec[:, 12:15], rec[:, 15:18], rec[:, 18:21] = N, V, L
    w = rec.view(np.uint32).copy()
    w[:, 21] = np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(12345) if seeds is None else np.asarray(seeds, np.uint32)
    return w


def material_of(words):
    rec = words.view(np.float32)
    m = dict(color=rec[:, 0:3].astype(np.float64))
    for c, key in enumerate(B.KEYS):
        m[key] = rec[:, 3 + c].astype(np.float64)
    return m


ALL_LOBES = dict(color=(0.8, 0.5, 0.3), specular=0.7, specular_tint=0.4, subsurface=0.3, sheen=0.6, sheen_tint=0.7, clearcoat=0.8, clearcoat_gloss=0.6)
PLAIN = dict(color=(0.8, 0.5, 0.3))
ROUGH_PEAK = (0.0, 0.0005, 0.001, 0.01, 0.05, 0.3, 1.0)


def _cat(parts):
    return np.concatenate(parts)


def _rotate_towards(R, T, delta):
    return np.cos(delta)[:, None] * R + np.sin(delta)[:, None] * T


def _perp(rng, R):
    T = rng.normal(size=R.shape)
    T -= (T * R).sum(-1, keepdims=True) * R
    return B._unit(T)


def _tilted_frames(rng, n):
    N = np.where((np.arange(n) % 2 == 0)[:, None], N_AXIS, B._unit(rng.normal(size=(n, 3))))
    return N


def _about(rng, N, cos):
    """unit vectors with N.v = cos (N unit)"""
    return cos[:, None] * N + np.sqrt(1.0 - cos * cos)[:, None] * _perp(rng, N)


def families():
    """name -> (n, 24) uint32 records.  Deterministic; shared with tests/test_gpu_bsdf_definition.py."""
    rng = np.random.default_rng(77)
    fam = {}
    # random: as _bsdf_records of tests/test_gpu_units.py, half with every lobe on
    n = 20000
    N = B._unit(rng.normal(size=(n, 3)))
    V = B._unit(N + 0.9 * B._unit(rng.normal(size=(n, 3))))
    L = B._unit(N * rng.uniform(-0.2, 1.0, (n, 1)) + B._unit(rng.normal(size=(n, 3))))
    mat = _random_lobes(rng, n)
    plain = np.arange(n) >= n // 2
    for key, v in (("specular", 0.5), ("specular_tint", 0.0), ("subsurface", 0.0), ("sheen", 0.0), ("sheen_tint", 0.5), ("clearcoat", 0.0), ("clearcoat_gloss", 1.0)):
        mat[key] = np.where(plain, v, mat[key])
    fam["random"] = records(mat, N, V, L, rng.integers(0, 2 ** 32, n, dtype=np.uint64))
    # axis normals: exact zeros, N.L exactly zero / positive / negative in any arithmetic
    s = math.sqrt(0.5)
    normals = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (s, 0, s)]
    dirs = [d for d in normals[:6]]
    for i, j in ((0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1)):
        for si in (0.6, -0.6):
            for sj in (0.8, -0.8):
                d = [0.0, 0.0, 0.0]; d[i], d[j] = si, sj
                dirs.append(tuple(d))
    w = 1.0 / math.sqrt(3.0)
    dirs += [(w, w, -w), (-w, w, w), (s, 0, -s), (-s, 0, s), (w, -w, -w)]      # N.L exactly 0 / of either sign for the tie normal
    dirs = np.array(dirs)
    iN, iV, iL = np.meshgrid(np.arange(len(normals)), np.arange(len(dirs)), np.arange(len(dirs)), indexing="ij")
    Nn, Vv, Ll = np.array(normals)[iN.ravel()], dirs[iV.ravel()], dirs[iL.ravel()]
    keep = np.abs(f32(Vv) + f32(Ll)).max(-1) > 0          # L = -V is the antipodal family's
    parts = []
    for base, metallic, rough in ((PLAIN, 0.0, 0.3), (ALL_LOBES, 0.5, 0.05), (ALL_LOBES, 1.0, 1.0), (PLAIN, 0.5, 0.0005)):
        parts.append(records(dict(base, metallic=metallic, roughness=rough), Nn[keep], Vv[keep], Ll[keep]))
    fam["axis normals"] = _cat(parts)
    # peak: L within 1e-4 ... 1e-1 rad of the mirror direction
    parts = []
    for rough in ROUGH_PEAK:
        for base in (PLAIN, ALL_LOBES):
            n = 300
            N = _tilted_frames(rng, n)
            V = _about(rng, N, rng.uniform(0.1, 1.0, n))
            R = 2.0 * (N * V).sum(-1, keepdims=True) * N - V
            L = _rotate_towards(R, _perp(rng, R), 10.0 ** rng.uniform(-4, -1, n))
            parts.append(records(dict(base, metallic=rng.choice([0.0, 0.5, 1.0], n), roughness=rough), N, V, L))
    fam["peak"] = _cat(parts)
    # grazing: N.V or N.L in {1e-6, 1e-4, 1e-2}
    parts = []
    for g in (1e-6, 1e-4, 1e-2):
        for base in (PLAIN, ALL_LOBES):
            for which in (0, 1):
                n = 200
                N = _tilted_frames(rng, n)
                a, b = _about(rng, N, np.full(n, g)), _about(rng, N, rng.uniform(0.05, 1.0, n))
                V, L = (a, b) if which == 0 else (b, a)
                parts.append(records(dict(base, metallic=rng.choice([0.0, 0.5, 1.0], n), roughness=rng.choice([0.0005, 0.05, 0.3, 1.0], n)), N, V, L))
    fam["grazing"] = _cat(parts)
    # retro: L = V, and L = V = N
    parts = []
    for base in (PLAIN, ALL_LOBES):
        n = 300
        N = _tilted_frames(rng, n)
        V = _about(rng, N, rng.uniform(0.02, 1.0, n))
        V[: n // 3] = N[: n // 3]
        parts.append(records(dict(base, metallic=rng.choice([0.0, 0.5, 1.0], n), roughness=rng.choice([0.0005, 0.05, 0.3, 1.0], n)), N, V, V))
    fam["retro"] = _cat(parts)
    # black / saturated base colours
    parts = []
    for color in ((0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
        for base in (PLAIN, ALL_LOBES):
            n = 200
            N, V, L = _random_geometry(rng, n)
            L = B._unit(L + 1.2 * N)
            parts.append(records(dict(base, color=color, metallic=rng.choice([0.0, 0.5, 1.0], n), roughness=rng.choice([0.0005, 0.05, 0.3, 1.0], n)), N, V, L))
    fam["black / saturated"] = _cat(parts)
    # ratio edges: metallic exactly 0, 0.5, 1
    parts = []
    for metallic in (0.0, 0.5, 1.0):
        for base in (PLAIN, ALL_LOBES):
            n = 300
            N, V, L = _random_geometry(rng, n)
            L = B._unit(L + 1.2 * N)
            parts.append(records(dict(base, metallic=metallic, roughness=rng.choice([0.0005, 0.05, 0.3, 1.0], n)), N, V, L, rng.integers(0, 2 ** 32, n, dtype=np.uint64)))
    fam["ratio edges"] = _cat(parts)
    # pinned seeds: all 256 seeds of each pinned draw
    top = (1 << 24) - 1
    for name, which, value in (("r2 = 0", 2, lambda dr: 0), ("r2 = 2^24 - 1", 2, lambda dr: top), ("r1 = 0", 1, lambda dr: 0), ("r1 = 2^24 - 1", 1, lambda dr: top),
                               ("probability = diffuseRatio", 0, lambda dr: int(dr * (1 << 24))), ("probability = diffuseRatio - 2^-24", 0, lambda dr: int(dr * (1 << 24)) - 1)):
        parts = []
        for metallic in (0.0, 0.5):
            seeds = B.seeds_pinning(which, value(0.5 * (1.0 - metallic)))
            for rough in (0.0005, 0.3, 1.0):
                for N in (N_AXIS, N_TILT, np.array([s, 0.0, s])):
                    V = view(N, 0.8)
                    L = view(N, 0.5, 2.0)
                    parts.append(records(dict(ALL_LOBES if rough == 0.3 else PLAIN, metallic=metallic, roughness=rough), np.tile(N, (256, 1)), np.tile(V, (256, 1)), np.tile(L, (256, 1)), seeds))
        fam["pinned " + name] = _cat(parts)
    return fam


def antipodal():
    """L = -V exactly: h = normalize(0) and Pdf is 0 / 0 in the formula itself."""
    rng = np.random.default_rng(78)
    n = 64
    N = _tilted_frames(rng, n)
    V = f32(_about(rng, N, rng.uniform(0.05, 1.0, n)))
    return records(dict(PLAIN, metallic=0.5, roughness=0.3), N, V, -V)


def definition(words):
    """The float64 outputs of every record: sampled direction, seed afterwards, Eval, Pdf, and the conditions (t2, t1) of the record's
    own L and of the sampler (see the module docstring), with the branch the sampler takes."""
    rec = words[:, :21].view(np.float32).astype(np.float64)
    mat = material_of(words)
    N, V, L = rec[:, 12:15], rec[:, 15:18], rec[:, 18:21]
    p, r1, r2, after = B.uniforms(words[:, 21])
    t2, t1 = B.condition(mat, N, V, L)
    a2 = B.specular_alpha(mat) ** 2
    diffuse = p < B.diffuse_ratio(mat)
    direction = B.sample(mat, N, V, p, r1, r2)
    den = 1.0 + (a2 - 1.0) * r2                                   # the sampler's two cancelling quantities: this denominator of cos^2 theta_h ...
    sin_h = np.sqrt(np.maximum(0.0, 1.0 - (1.0 - r2) / den))      # ... and 1 - cos^2 theta_h, whose root carries 2^-24 / (2 sin theta_h)
    value = B.pdf(mat, N, V, L)
    with np.errstate(invalid="ignore", divide="ignore"):         # Pdf's scale: its terms with the cosine factors at 1 (a dot product of unit vectors
        h = B._unit(L + V)                                         # carries an ABSOLUTE 2^-24) and the GTR1 term at full weight (lerp(g1, g2, k) = g1 + (g2 - g1) k
        c = np.abs((N * h).sum(-1))                                # passes g1 through FP32 even at clearcoat = 0, k = 1)
        dr = B.diffuse_ratio(mat)
        pdf_scale = dr / np.pi + (1.0 - dr) * (B.gtr2(c, B.specular_alpha(mat)) + B.gtr1(c, B.clearcoat_alpha(mat))) / (4.0 * np.abs((L * h).sum(-1)))
        f = B.eval(mat, N, V, L)
        g = (0.5 + 0.5 * mat["roughness"]) ** 2                   # Eval's scale: its largest component, or what the absolute 2^-24 of L.h moves the Schlick weight
        nl, nv = (N * L).sum(-1), (N * V).sum(-1)                 # (1 - L.h)^5 of the specular lobe by, 5 (1 - L.h)^4 D2 G, where that is larger (a black metal)
        lobe = B.gtr2((N * h).sum(-1), B.specular_alpha(mat)) * B._g1(nl, g) * B._g1(nv, g) / (4.0 * nl * nv)
        f_scale = np.maximum(np.abs(f).max(-1), np.where((nl > 0) & (nv > 0), 5.0 * np.clip(1.0 - (L * h).sum(-1), 0.0, 1.0) ** 4 * lobe, 0.0))
    return dict(mat=mat, N=N, V=V, L=L, dir=direction, seed=after, f=f, f_scale=f_scale, pdf=value, pdf_scale=pdf_scale, t2=t2, t1=t1,
                t2_dir=np.where(diffuse, np.sqrt(1.0 - r1), den * sin_h), diffuse=diffuse, r1=r1, coat=mat["clearcoat"] != 0.0)


def errors(d, direction, f, pdf):
    """Per record, in units of 2^-24 scale: (direction, Eval, Pdf).  A zero reference admits only a zero."""
    def unit_err(got, want, scale):
        got = np.asarray(got, np.float64)
        e = np.abs(got - want)
        e = e.max(-1) if e.ndim > 1 else e
        with np.errstate(divide="ignore", invalid="ignore"):
            out = np.where(scale > 0, e / (scale * EPS32), np.where(e == 0, 0.0, np.inf))
        return np.where(np.isnan(out), np.inf, out)
    return (unit_err(direction, d["dir"], np.ones(len(d["pdf"]))), unit_err(f, d["f"], d["f_scale"]), unit_err(pdf, d["pdf"], d["pdf_scale"]))


def bound(d, which):
    """The bound of the module docstring in units of 2^-24 scale, for output `which` (0 direction, 1 Eval, 2 Pdf)."""
    t2 = d["t2_dir"] if which == 0 else d["t2"]
    coat = d["coat"] & (which != 0)             # Sample draws no clearcoat lobe
    with np.errstate(divide="ignore"):
        return C0 + C2 / t2 + np.where(coat, C1 / d["t1"], 0.0)


def random_mask(d):
    """The records of the random family that are judged: |N.L| and |N.V| at least 1e-6 in float64."""
    return (np.abs((d["N"] * d["L"]).sum(-1)) >= 1e-6) & (np.abs((d["N"] * d["V"]).sum(-1)) >= 1e-6)


def report(side, name, errs):
    e = np.maximum.reduce(errs)
    q = np.quantile(e, [0.5, 0.99, 1.0])
    worst = " ".join(f"{x.max():.3g}" for x in errs)
    print(f"{side}: {name:36s} n = {len(e):6d}  error / (2^-24 scale) 50 / 99 / 100 % = {q[0]:.3g} / {q[1]:.3g} / {q[2]:.3g}   (worst direction, Eval, Pdf: {worst})")


def oracle_outputs(ob, words):
    """The oracle's Sample, Eval, Pdf of every record (one call per distinct material)."""
    rec = words.view(np.float32)
    n = len(rec)
    direction, f, pdf, after = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint32)
    _, inverse = np.unique(words[:, :12], axis=0, return_inverse=True)
    inverse = inverse.ravel()
    order = np.argsort(inverse, kind="stable")
    bounds = np.flatnonzero(np.diff(inverse[order])) + 1
    for idx in np.split(order, bounds):
        r = rec[idx[0]]
        m = dict(color=tuple(float(x) for x in r[0:3]), **{key: float(r[3 + c]) for c, key in enumerate(B.KEYS)})
        direction[idx], after[idx] = ob.bsdf_sample(m, rec[idx, 12:18], words[idx, 21])
        f[idx], pdf[idx] = ob.bsdf_eval_pdf(m, rec[idx, 12:21])
    return direction, after, f, pdf


def fit_constants(samples):
    """samples: (error, t2, t1, coat) arrays per family and output.  C0 puts the worst record without clearcoat and with t2 >= 1/2 at
    half the bound, then C2 the worst of all records without clearcoat, then C1 the worst with clearcoat."""
    e, t2, t1, coat = (np.concatenate([s[i] for s in samples]) for i in range(4))
    well = ~coat & (t2 >= 0.5)
    c0 = 2.0 * float(e[well].max())
    c2 = max(0.0, float(((2.0 * e[~coat] - c0) * t2[~coat]).max()))
    c1 = max(0.0, float(((2.0 * e[coat] - c0 - c2 / t2[coat]) * t1[coat]).max()))
    return c0, c2, c1


def round_up(x):
    if x <= 0:
        return 0.0
    k = 10.0 ** math.floor(math.log10(x))
    return math.ceil(x / k - 1e-9) * k


def judge(side, outputs):
    """For every family: the exact checks, then the printed quantiles; returns the per-output samples (error, t2, t1, coat) and the
    failures of the bound and of the 1e-5 bar, so that a caller prints everything before it asserts.  outputs(words) -> direction,
    seed afterwards, Eval, Pdf."""
    samples, failures = [], []
    for name, words in families().items():
        d = definition(words)
        direction, after, f, pdf = outputs(words)
        assert np.array_equal(after, d["seed"]), name                     # three draws of the integer LCG
        assert np.isfinite(direction).all() and np.isfinite(f).all() and np.isfinite(pdf).all(), name
        keep = np.ones(len(words), bool)
        if name == "random":
            keep = random_mask(d)
            assert (~keep).sum() <= 1e-4 * len(keep)
        if name == "axis normals":                                         # the products are exact there, in FP32 as in float64
            dead = ((d["N"] * d["L"]).sum(-1) <= 0) | ((d["N"] * d["V"]).sum(-1) <= 0)
            assert dead.sum() > 1000 and (np.asarray(f)[dead] == 0).all()
        if name.startswith("pinned"):                                      # the branch, read off the direction: a cosine sample has x^2 + y^2 = r1 in the N frame
            c, _ = B.local(d["N"], np.asarray(direction, np.float64))
            disk = np.abs((1.0 - c * c) - d["r1"]) <= 1e-5
            assert np.array_equal(disk, d["diffuse"]), name
            if "probability = diffuseRatio" in name:
                assert d["diffuse"].all() == name.endswith("2^-24") and d["diffuse"].any() == name.endswith("2^-24")
        errs = [e[keep] for e in errors(d, direction, f, pdf)]
        report(side, name, errs)
        for which, e in enumerate(errs):
            t2 = (d["t2_dir"] if which == 0 else d["t2"])[keep]
            coat = (d["coat"] & (which != 0))[keep]
            samples.append((e, t2, d["t1"][keep], coat))
            b = bound(d, which)[keep]
            worst = int(np.argmax(e / b))
            if not (e <= b).all():
                failures.append((name, ("direction", "Eval", "Pdf")[which], "bound", float(e[worst]), float(b[worst])))
            easy = ~d["coat"][keep] & (d["t2"][keep] >= 0.05)              # the all-lobes code against its second writing: 1e-5 where FP32 is well conditioned
            if which != 0 and not (e[easy] * EPS32 <= 1e-5).all():
                failures.append((name, ("direction", "Eval", "Pdf")[which], "1e-5 at t2 >= 0.05 without clearcoat", float(e[easy].max() * EPS32)))
    return samples, failures


def test_oracle_against_the_definition(ob):
    """Every family, every record: finite, the seed the integer LCG's, Eval exactly zero where N.L or N.V is exactly <= 0, the pinned
    seeds on the definition's branch, and direction / Eval / Pdf inside the bound with the constants of the module docstring, which
    this test re-measures."""
    samples, failures = judge("oracle", lambda words: oracle_outputs(ob, words))
    c0, c2, c1 = fit_constants(samples)
    print(f"oracle: fitted C0 = {c0:.3g}, C2 = {c2:.3g}, C1 = {c1:.3g} -> rounded up {round_up(c0):g}, {round_up(c2):g}, {round_up(c1):g}; in use {C0:g}, {C2:g}, {C1:g}")
    assert not failures, failures
    assert (round_up(c0), round_up(c2), round_up(c1)) == (C0, C2, C1)


def test_pdf_of_the_opposite_direction_is_not_a_number(ob):
    """L = -V: normalize(L + V) divides zero by zero, in the definition as in the oracle -- written down, not fixed: Sample returns
    -V only for V.h = 0 exactly and the walks reject a non-finite pdf."""
    words = antipodal()
    d = definition(words)
    _, _, f, pdf = oracle_outputs(ob, words)
    assert not np.isfinite(pdf).any() and not np.isfinite(d["pdf"]).any()
    assert (f == 0).all() and (d["f"] == 0).all()          # Eval leaves on N.L <= 0 or N.V <= 0 before it forms h
