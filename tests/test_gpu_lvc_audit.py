"""Every record of the DEVICE's light-vertex cache recomputed in float64 from the record stored before it (tests/lvc_audit.py).

k_light_trace (csrc/kernels_light.hip) builds its vertices inline -- pdf_G, flux, single_pdf, pdf, last_lum, the tracing_init_light /
tracing_update_light recursion of rmis_pointer -- in a persistent, lane-regenerating loop whose per-path state lives in registers
across path and core boundaries.  tests/test_gpu_parity.py::check_lvc compares the cache with the oracle's up to the first
Russian-roulette flip at the 99th percentile below 1e-3; here 100 % of the records of every scenario are judged on their own: the
structure of the cache, the origin vertices against the light's geometry, every step's geometry (the hit lies in a triangle of its
material, the segment crosses no other triangle), the measures and the throughput, the RMIS recursion and the subspace labels.
A value left over from the lane's previous path, or a wrong exit where a core's slot range fills, shows as named records.

Bars (lvc_audit.BARS, C_KAPPA = 2): `bar + 2 kappa` for the 99.9 % quantile and `hard + 2 kappa` on every record, kappa the record's
own conditioning number; each bar is 4 x what the ORACLE's cache measures under the same audit on the CPU (24 caches: the four
scenarios of tests/test_lvc_audit_cpu.py at six launch frames), floored at 2e-6 -- never a margin over the device's own figures.
Figures are max(err - 2 kappa, 0) over the well-conditioned records, 99.9 % quantile / maximum, largest over the scenarios:

  field                      bar 99.9 % / hard     oracle (CPU, measured)    device (MI355X, measured: the 13 caches of this module)
  origin pdf                 2e-6    / 2e-6        0 / 0 (the FP32 quotient)  0 / 0
  origin pdf (sky)           8.4e-4  / 1e-3        2.1e-4 / 2.5e-4           2.0e-4 / 2.5e-4
  pdf                        2e-6    / 2e-6        0 / 0 (the FP32 product)   0 / 0
  last_lum                   2e-6    / 2e-6        1.5e-7 / 1.7e-7           1.5e-7 / 1.8e-7
  last_normal_projection     2e-6    / 3.4e-6      2.3e-7 / 8.4e-7           1.9e-7 / 6.2e-7
  single_pdf depth 1         2e-6    / 1.4e-5      2.2e-7 / 3.5e-6           3.5e-7 / 3.4e-6
  flux depth 1               2e-6    / 1.4e-5      1.9e-7 / 3.5e-6           2.8e-7 / 3.3e-6
  single_pdf depth >= 2      1.24e-4 / 7.6e-4      3.1e-5 / 1.9e-4           2.8e-5 / 5.6e-5
  flux depth >= 2            1.24e-4 / 7.6e-4      3.1e-5 / 1.9e-4           2.9e-5 / 5.7e-5
  rmis_pointer depth >= 2    1.84e-4 / 8e-4        4.6e-5 / 2.0e-4           1.6e-5 / 5.0e-5
  ill-conditioned share      <= 0.5 % of a cache   0.34 %                    0.15 %
c = 2 is the largest power of two at which the oracle stays inside the 0.5 % cap on all 24 caches (0.54 % at c = 4).  A record whose
2 kappa exceeds 1e-2 (a few-millimetre segment, the 0.05-roughness metal, a walk that runs nearly straight through a surface) is
held to a flat 5e-2 (to 2 kappa alone where that exceeds 5e-2: the oracle holds records at 0.054 and 0.12 there, 0.33 of their 2 kappa at
most over 48 caches; the device's cornell frame 8 holds the oracle's 0.054 record, digit for digit) and counted against the cap; where an ulp moves the value by half of itself the formula has a pole within
rounding (L ~ -V: 1 / |L . H|) and no bound holds: counted against the cap and printed, not judged (at most 10 such records in the
13 device caches of 144 000 records).  No error was found in k_light_trace.
Sky origins: flux against the float64 bilinear lookup of tests/env_ref.py within 1e-6 (u, v) x the cell's slope + 2e-6 of its largest
texel (measured on the device: 0.06 of that bar); pdf not judged within 1e-4 texel of a texel border, at most 1e-3 of them, counted.
Exact, no tolerance: the structure (predecessor rule, path ids, slot ranges, path count, depth <= 52), the flags, last_position,
last_zone_id, material_id, the untextured colour, rmis_pointer at depth 1, the origin's flux / rmis_pointer; labels within rounding
of a split or a patch border: at most 1e-3 of the records.  Every scenario prints its quantiles (run with -s)."""
import numpy as np
import pytest

from tests import lvc_audit as A
from tests.parity_util import cornell_with_flagged_box, minimal_tuple

pytestmark = pytest.mark.gpu


def _renderer(pkg, scene, lt, decorrelate=None):
    r = pkg.Renderer(scene, 0)
    cam = scene.camera
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], 1.0)
    r.resize(64, 64)
    if scene.environment is not None:
        r.set_environment(scene.environment["rgba"], scene.environment["center"], scene.environment["radius"])
    r.set_light_trace(*lt, decorrelate=decorrelate)
    return r


def _minimal(pkg, ob, scene, r, lt):
    """minimal_tuple of the oracle on the same scene and launch geometry, installed on the device"""
    o = ob.Oracle(scene)
    cam = scene.camera
    o.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], 1.0)
    o.resize(8, 8)
    if scene.environment is not None:
        o.set_environment(scene.environment["rgba"], scene.environment["center"], scene.environment["radius"])
    o.set_light_trace(*lt)
    r.set_subspace(*minimal_tuple(o, 2))


def _audit(r, scene, lt, name, frame=7, lvc=None, paths=None):
    """One light pass of the device, audited record by record; the tuple is read back from the device."""
    if lvc is None:
        r.launch("light trace", frame)
        lvc = r.lvc_read()
        r.build_sampler()
        paths = r.sampler_read()[4]
    assert len(lvc) > 1000, name
    res = A.audit(scene, r.get_subspace(), lvc, lt, env=scene.environment, path_count=paths)
    fails = A.judge(res, lvc, name)
    assert not fails, "\n".join(m for _, m in fails)
    n_step = len(res["last_lum"].err)
    assert n_step + len(res["origin: position"].err) == len(lvc), name        # 100 % of the records judged: origins + steps = the cache
    assert len(res["single_pdf"].err) + len(res["single_pdf depth 1"].err) == n_step and len(res["rmis_pointer"].err) == len(res["flux"].err)
    return res, lvc


@pytest.mark.parametrize("decorrelate", [False, True])
def test_cornell_base_case(gpu, pkg, ob, decorrelate):
    scene, lt = pkg.scenes.cornell_box(), (3000, 64, 2)
    r = _renderer(pkg, scene, lt, decorrelate=decorrelate)
    _minimal(pkg, ob, scene, r, lt)
    _audit(r, scene, lt, f"cornell (3000, 64, 2), lt_decorrelate {int(decorrelate)}")


def test_cornell_many_paths_per_core_slot_ranges_fill(gpu, pkg, ob):
    """Cores end because their slot range is full, in the middle of a path and right after an origin: where per-path state left in
    the lane's registers would show."""
    scene, lt = pkg.scenes.cornell_box(), (60, 48, 40)
    r = _renderer(pkg, scene, lt)
    _minimal(pkg, ob, scene, r, lt)
    res, lvc = _audit(r, scene, lt, "cornell (60, 48, 40)")
    core = lvc["path_id"] // lt[2]
    full = np.bincount(core, minlength=lt[0]) == lt[1]
    last = np.concatenate([core[1:] != core[:-1], [True]]) & full[core]
    assert full.sum() > 10 and (lvc["depth"][last] == 0).any() and (lvc["depth"][last] > 0).any()


@pytest.fixture(scope="module")
def trained(gpu, pkg):
    """The product's own trained tuple: multi-leaf trees, Gamma != Q."""
    scene, lt = pkg.scenes.cornell_box(), (3000, 64, 1)
    r = _renderer(pkg, scene, lt)
    r.set_pretrace(20000, 10)
    r.preprocess(target_paths=100000, target_q_paths=100000, train=True)
    return r, scene, lt


@pytest.mark.parametrize("counting", [False, True])
def test_cornell_trained_tuple(trained, counting):
    """The RMIS recursion and the labels are non-trivial; the cache-filling (timed) pass and the counting pass are different
    instantiations of the kernel (labels cached in the vertex / descended again in the reference's order)."""
    r, scene, lt = trained
    r.enable_counters(counting)
    try:
        res, lvc = _audit(r, scene, lt, f"cornell (3000, 64, 1), trained tuple, counters {int(counting)}")
    finally:
        r.enable_counters(False)
    et, ltree, q, cmf = r.get_subspace()
    assert len(np.unique(lvc["subspace_id"][lvc["depth"] > 0])) > 20 and len(ltree) > 50
    st = res["_step"]
    assert np.ptp(st["S"]["gamma"][st["deep"]]) > 0                                  # Gamma / Q varies over the records


def test_bedroom_textured(gpu, pkg, ob):
    """Textured colours feed rr, Pdf and Eval; twelve Disney materials; two quad lights (n_lights = 2 in the origin pdf)."""
    scene, lt = pkg.scenes.bedroom(target_tris=8000, tex_size=64), (2000, 64, 1)
    r = _renderer(pkg, scene, lt)
    _minimal(pkg, ob, scene, r, lt)
    res, lvc = _audit(r, scene, lt, "bedroom (2000, 64, 1)")
    org = lvc[lvc["depth"] == 0]
    assert set(org["material_id"].tolist()) == {0, 1}
    tex = np.array([m.get("albedo_tex", 0) > 0 for m in scene.materials])
    assert tex[lvc["material_id"][res["_step"]["li"]][res["_step"]["deep"]]].sum() > 300    # textured predecessors


def test_courtyard_environment_map(gpu, pkg, ob):
    """DIRECTION origins on the sky disk, LAST_DIRECTION successors, the `lld` branch of rmis_last_pdf."""
    scene, lt = pkg.scenes.courtyard(), (8000, 64, 1)
    r = _renderer(pkg, scene, lt)
    _minimal(pkg, ob, scene, r, lt)
    res, lvc = _audit(r, scene, lt, "courtyard, sky (8000, 64, 1)")
    lld = (lvc["pad"] & A.LV_LAST_DIRECTION) != 0
    st = res["_step"]
    assert len(res["origin pdf (sky)"].err) > 500 and lld.sum() > 100 and (lld[st["li"]] & st["deep"]).sum() > 50


@pytest.mark.parametrize("which", ["cornell_sphere_lamp", "lamp_floor"])
def test_mesh_light_origins(gpu, pkg, which):
    scene, lt = getattr(pkg.scenes, which)(), (3000, 64, 1)
    r = _renderer(pkg, scene, lt)
    r.set_subspace()
    res, lvc = _audit(r, scene, lt, f"{which} (3000, 64, 1), mesh light")
    assert len(np.unique(lvc["subspace_id"][lvc["depth"] == 0])) == scene.mesh_lights[0]["n_patches"]


def test_cornell_brdf_flagged_walls(gpu, pkg, ob):
    """brdf_div in next_flux: the white walls and the short box carry `brdf 1`, roughness 0.5."""
    scene, lt = cornell_with_flagged_box(pkg, roughness=0.5, flag_walls=True), (3000, 64, 2)
    r = _renderer(pkg, scene, lt)
    _minimal(pkg, ob, scene, r, lt)
    res, lvc = _audit(r, scene, lt, "cornell, brdf-flagged walls (3000, 64, 2)")
    st = res["_step"]
    assert (st["S"]["mat"]["brdf"][st["deep"]] != 0).sum() > 1000


def test_batched_light_passes(gpu, pkg, ob, monkeypatch):
    """launch_light_batch: three frames' passes through one core queue -- a different path through the regeneration code; every
    frame's cache audited on its own."""
    import torch
    monkeypatch.setenv("SPCBPT_SETS", "7")
    scene, lt = pkg.scenes.cornell_box(), (3000, 64, 2)
    r = _renderer(pkg, scene, lt)
    _minimal(pkg, ob, scene, r, lt)
    r.set_light_ahead(True)
    r.launch_light_batch(7, 3)
    dev = torch.device("cuda", 0)
    seen = []
    for f in range(3):
        r.sync_light()
        dv, dc, cap = r.lvc_export()                                    # the oldest pass that has no sampler yet
        n, paths = pkg.dist.device_view(dc, 8, dev).view(torch.int32).cpu().numpy()
        lvc = pkg.dist.device_view(dv, int(n) * 96, dev).cpu().numpy().view(pkg.api.LIGHT_VERTEX_DTYPE).copy()
        _audit(r, scene, lt, f"cornell (3000, 64, 2), frame {7 + f} of a batch of 3", lvc=lvc, paths=int(paths))
        seen.append(lvc["position"][:64].tobytes())
        r.build_sampler()
    assert len(set(seen)) == 3                                           # three different passes
