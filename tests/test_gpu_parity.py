"""Parity of the HIP path (through the C ABI) against the oracle on the same seeded inputs.

Tolerances (all floating point is FP32; since round 3 the device code is compiled without implicit FMA fusion, like the oracle, so
the two differ by transcendental ulps, the traversal loop's v_rcp_f32 / explicit FMAs and BVH tie-breaking only; equality is still
statistical at the path level -- one Russian-roulette decision within rounding of its threshold gives a pixel another sample -- and
tight at the function level):
  * traversal: same triangle, |dt| <= 1e-5 * max(1, t) for >= 99.9 % of rays (ties at shared edges excepted)
  * light-vertex cache: same (path_id, depth) sequence; values within 1e-3 relative for >= 99 % of vertices
  * sampler tables: integers exact; CMFs within 3e-5 absolute (device scan accumulates in double, the reference in float)
  * images, same seeds: >= 99.7 % of pixels (measured 99.89 ... 100 %; round 2: 99 %) within 2e-3 relative + 1e-4 absolute per channel when the oracle runs with the
    product's CMF accumulation precision; image mean within 0.5 %; with the reference's float CMFs the per-pixel L2
    difference must stay below 25 % of the Monte-Carlo RMSE at that sample count.
"""
import numpy as np
import pytest

from tests.parity_util import image_parity, tails_explained, minimal_tuple, rmse

pytestmark = pytest.mark.gpu


def _pair(pkg, ob, scene, w, h, lt=(2000, 64, 1)):
    r = pkg.Renderer(scene, 0)
    o = ob.Oracle(scene)
    cam = scene.camera
    for x in (r, o):
        x.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
        x.resize(w, h)
        x.set_light_trace(*lt)
    return r, o


def _rays(rng, n, lo, hi, tmax=1e16):
    org = rng.uniform(lo, hi, size=(n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tm = np.full((n, 1), tmax, np.float32) if np.isscalar(tmax) else tmax.reshape(n, 1).astype(np.float32)
    return np.concatenate([org, np.full((n, 1), 1e-3, np.float32), d, tm], 1)


@pytest.mark.parametrize("scene_name,kw", [("cornell_box", {}), ("simple_room", {"n": 6}), ("bedroom", {"target_tris": 60000, "tex_size": 64})])
def test_traversal_matches_oracle_bvh(gpu, pkg, ob, scene_name, kw):
    scene = getattr(pkg.scenes, scene_name)(**kw)
    r, o = _pair(pkg, ob, scene, 8, 8)
    lo, hi = scene.vertices.min(0) + 0.05, scene.vertices.max(0) - 0.05
    rays = _rays(np.random.default_rng(1), 50000, lo, hi)
    t0, tri0, uv0 = o.trace_closest(rays)
    t1, tri1, uv1 = r.trace_closest(rays)
    same = tri0 == tri1
    assert same.mean() >= 0.999
    assert (np.abs(t0 - t1)[same] <= 1e-5 * np.maximum(1.0, t0[same])).all()
    hit = same & (tri0 >= 0)
    assert np.abs(uv0 - uv1)[hit].max() < 1e-3
    # quad-light triangles are reported after the scene's own triangles
    assert tri1.max() < len(scene.indices) + 2 * len(scene.lights)
    rays2 = _rays(np.random.default_rng(2), 50000, lo, hi, tmax=np.random.default_rng(3).uniform(0.05, 4.0, 50000))
    v0, v1 = o.trace_any(rays2), r.trace_any(rays2)
    assert (v0 == v1).mean() >= 0.999


def test_emitter_quads_are_single_sided_for_path_rays_only(gpu, pkg, ob):
    """closest-hit rays pass through the back of a light quad, shadow rays do not."""
    scene = pkg.scenes.cornell_box()
    r, o = _pair(pkg, ob, scene, 8, 8)
    up = np.array([[0, 1.0, 0, 1e-3, 0, 1, 0, 1e16]], np.float32)      # from below: front face (normal is -y)
    down = np.array([[0, 1.9995, 0, 1e-4, 0, -1, 0, 1e16]], np.float32)  # from the 2 mm gap above the light
    n_scene = len(scene.indices)
    for x in (o, r):
        t, tri, _ = x.trace_closest(up)
        assert tri[0] >= n_scene and abs(t[0] - 0.998) < 1e-4
        t, tri, _ = x.trace_closest(down)
        assert tri[0] < n_scene          # culled: continues to the floor
        vis = x.trace_any(np.array([[0, 1.9995, 0, 1e-4, 0, -1, 0, 1.0]], np.float32))
        assert vis[0] == 0               # but it occludes a shadow ray


@pytest.mark.parametrize("lt", [(3000, 64, 2), (60, 48, 40)])
def test_light_vertex_cache_matches_oracle(gpu, pkg, ob, lt):
    """(3000, 64, 2): two paths per core, ranges never fill.  (60, 48, 40): the reference's kind of geometry -- many paths per
    core, and most cores end because their padded slot range is full (raygen.cu:652, 676), in the middle of a path or right
    after an origin vertex; the persistent light kernel must cut every core at the same vertex as the per-core loop."""
    check_lvc(pkg, ob, pkg.scenes.cornell_box(), lt)


def check_lvc(pkg, ob, scene, lt):
    """The device's cache against the oracle's at the same seeds: the same (path_id, depth) sequence and the oracle's VALUES on the
    common prefix up to the first Russian-roulette / tie flip (at least half of the cache), at the 99th percentile.  That the walk draws
    the oracle's random numbers and lands where the oracle lands is only held here.  What every single record holds -- each field
    recomputed in float64 from the record stored before it, behind the first flip too, with a hard bar on every record -- is the audit of
    tests/test_gpu_lvc_audit.py."""
    r, o = _pair(pkg, ob, scene, 8, 8, lt=lt)
    tup = minimal_tuple(o, 2)
    r.set_subspace(*tup); o.set_subspace(*tup)
    r.launch("light trace", 7); o.launch("light trace", 7)
    a, b = r.lvc_read(), o.lvc_read()
    n = min(len(a), len(b))
    assert abs(len(a) - len(b)) <= 0.002 * len(b)
    same = (a["path_id"][:n] == b["path_id"][:n]) & (a["depth"][:n] == b["depth"][:n])
    first_div = n if same.all() else int(np.argmin(same))
    assert first_div >= 0.5 * n  # a rare RR/tie flip shifts everything after it; compare the common prefix
    a, b = a[:first_div], b[:first_div]
    assert (a["subspace_id"] == b["subspace_id"]).mean() > 0.999
    surf = a["depth"] > 0   # origin vertices carry stale ring-slot data in these fields in the reference (never read)
    assert (a["material_id"] == b["material_id"]).all() and (a["last_zone_id"] == b["last_zone_id"])[surf].mean() > 0.999
    for k in ("position", "flux", "pdf", "single_pdf", "rmis_pointer", "last_lum", "color", "last_normal_projection"):
        sel = surf if k in ("last_lum", "color", "last_normal_projection") else slice(None)
        x, y = a[k][sel].astype(np.float64), b[k][sel].astype(np.float64)
        scale = np.abs(y).max(axis=-1, keepdims=True) if y.ndim > 1 else np.abs(y)
        rel = np.abs(x - y) / (scale + 1e-9)
        assert np.percentile(rel, 99) < 1e-3, k
    assert (np.abs((a["normal"] * b["normal"]).sum(1) - 1) < 1e-5).mean() > 0.999
    return a, b


def test_sampler_tables_exact_on_identical_lvc(gpu, pkg, ob):
    """LVC_Process on the device: integer tables bit-exact, CMFs within the double-vs-float accumulation gap."""
    scene = pkg.scenes.cornell_box()
    r, o = _pair(pkg, ob, scene, 8, 8, lt=(4000, 64, 1))
    tup = minimal_tuple(o, 2)
    r.set_subspace(*tup); o.set_subspace(*tup)
    o.launch("light trace", 3)
    lvc = o.lvc_read()
    r.lvc_import(lvc)
    r.build_sampler(); o.build_sampler()
    sg, so = r.sampler_read(), o.sampler_read()
    assert sg[3:] == so[3:]
    np.testing.assert_array_equal(sg[0]["size"], so[0]["size"])
    np.testing.assert_array_equal(sg[0]["jump_bias"], so[0]["jump_bias"])
    np.testing.assert_array_equal(sg[2], so[2])
    assert np.abs(sg[1] - so[1]).max() < 3e-5
    np.testing.assert_allclose(sg[0]["sum_pmf"], so[0]["sum_pmf"], rtol=1e-4)
    o.set_cmf_double(True); o.build_sampler()
    np.testing.assert_allclose(sg[1], o.sampler_read()[1], rtol=0, atol=2e-7)
    # golden: committed oracle tables for a fixed LVC
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "oracle_cornell32.npz"))
    r.lvc_import(g["lvc"]); r.build_sampler()
    sub, cmfs, jump, vc, pc = r.sampler_read()
    assert (vc, pc) == (int(g["vc"]), int(g["pc"]))
    np.testing.assert_array_equal(jump, g["jump"])
    np.testing.assert_array_equal(sub["size"], g["sub"]["size"])
    assert np.abs(cmfs - g["cmfs"]).max() < 3e-5


def test_sampler_edge_cases(gpu, pkg, ob):
    """Empty LVC, single vertex, all-zero-weight subspace (SURVEY q11 guard)."""
    scene = pkg.scenes.cornell_box()
    r, o = _pair(pkg, ob, scene, 8, 8, lt=(100, 8, 1))
    tup = minimal_tuple(o, 1)
    r.set_subspace(*tup)
    o.launch("light trace", 1)
    lvc = o.lvc_read()
    r.lvc_import(lvc[:0] if len(lvc) == 0 else lvc[:1]); r.build_sampler()
    sub, cmfs, jump, vc, pc = r.sampler_read()
    assert vc == 1 and cmfs[0] == 1.0 and jump[0] == 0 and sub["size"].sum() == 1
    z = lvc[:5].copy()
    z["flux"] = 0
    z["subspace_id"] = 17
    r.lvc_import(z); r.build_sampler()
    sub, cmfs, jump, vc, pc = r.sampler_read()
    assert sub["size"][17] == 5 and np.isfinite(cmfs).all() and cmfs[4] == 1.0 and (np.diff(cmfs) > 0).all()


@pytest.mark.parametrize("scene_name", ["cornell_box", "simple_room"])
def test_pt_image_matches_oracle(gpu, pkg, ob, scene_name):
    scene = getattr(pkg.scenes, scene_name)()
    r, o = _pair(pkg, ob, scene, 96, 64)
    for f in range(4):
        r.launch("pt", f); o.launch("pt", f)
    s = image_parity(r.read_accum()[..., :3], o.read_accum()[..., :3])
    assert s["frac_close"] >= 0.998 and s["mean_rel"] < 5e-3 and tails_explained(s), s
    fa, fb = r.read_frame(), o.read_frame()
    assert (np.abs(fa.astype(int) - fb.astype(int)) <= 1).mean() > 0.99   # tone-mapped sRGB bytes


@pytest.mark.parametrize("scene_name", ["cornell_box", "simple_room"])
def test_spcbpt_image_matches_oracle(gpu, pkg, ob, scene_name):
    scene = getattr(pkg.scenes, scene_name)()
    r, o = _pair(pkg, ob, scene, 96, 64)
    tup = minimal_tuple(o, 2)
    r.set_subspace(*tup); o.set_subspace(*tup)
    o.set_cmf_double(True)   # match the product's CMF accumulation precision (see module docstring)
    for f in range(4):
        r.render_frame("SPCBPT_eye", f); o.render_frame("SPCBPT_eye", f)
    a = r.read_accum()[..., :3]
    s = image_parity(a, o.read_accum()[..., :3])
    assert s["frac_close"] >= 0.997 and s["mean_rel"] < 5e-3 and tails_explained(s), s
    # against the reference-exact float CMFs: differences are far below the Monte-Carlo noise
    o.set_cmf_double(False); o.clear_accum()
    for f in range(4):
        o.render_frame("SPCBPT_eye", f)
    b = o.read_accum()[..., :3]
    o.clear_accum()
    for f in range(100, 164):
        o.render_frame("SPCBPT_eye", f)   # independent higher-spp estimate -> MC noise level
    ref = o.read_accum()[..., :3]
    assert rmse(a, b) < 0.25 * rmse(b, ref), (rmse(a, b), rmse(b, ref))
    assert abs(a.mean() - b.mean()) / b.mean() < 5e-3



def test_spcbpt_with_multi_leaf_trees_and_textures(gpu, pkg, ob):
    """Classification, stage-1 sampling over many light subspaces and textured materials, on a bedroom-class scene."""
    from tests.parity_util import grid_tree_tuple
    scene = pkg.scenes.bedroom(target_tris=40000, tex_size=64)
    r, o = _pair(pkg, ob, scene, 64, 48, lt=(4000, 64, 1))
    tup = grid_tree_tuple(pkg, o, scene)
    r.set_subspace(*tup); o.set_subspace(*tup)
    o.set_cmf_double(True)
    o.set_skip_null_connections(True)   # count what the product counts (d10); the images agree with the knob on or off
    r.enable_counters(True); r.reset_counters(); o.reset_counters()
    for f in range(2):
        r.render_frame("SPCBPT_eye", f); o.render_frame("SPCBPT_eye", f)
    s = image_parity(r.read_accum()[..., :3], o.read_accum()[..., :3])
    assert s["frac_close"] >= 0.997 and s["mean_rel"] < 1e-2 and tails_explained(s), s
    cg, co = r.counters(), o.counters()
    for k in ("closest_rays", "shadow_rays", "surface_vertices", "connections", "textured_hits", "lvc_stores", "cmf_probes",
              "tree_nodes", "gamma_q_reads", "pixel_samples", "eye_paths", "light_paths"):
        assert abs(cg[k] - co[k]) <= 0.01 * max(co[k], 1) + 2, (k, cg[k], co[k])
    assert cg["textured_hits"] > 0 and cg["tree_nodes"] > cg["surface_vertices"]


def test_row_bands_and_lvc_sharding_are_rank_count_invariant(gpu, pkg, ob):
    """Multi-GPU decomposition on one GPU: 2 'ranks' trace half the cores each, shards concatenate to the single-rank
    LVC bit-exactly, and interleaved 8-row bands tile the image exactly."""
    scene = pkg.scenes.cornell_box()
    r, o = _pair(pkg, ob, scene, 64, 48, lt=(2000, 64, 1))
    tup = minimal_tuple(o, 1)
    r.set_subspace(*tup)
    r.launch("light trace", 5)
    full = r.lvc_read()
    shards = []
    for k in range(2):
        r.set_light_trace(2000, 64, 1, core_begin=1000 * k, core_count=1000)
        r.launch("light trace", 5)
        shards.append(r.lvc_read())
    cat = np.concatenate(shards)
    assert cat.tobytes() == full.tobytes()
    r.lvc_import(cat); r.build_sampler()
    r.launch("SPCBPT_eye", 0)
    whole = r.read_accum().copy()
    r.clear_accum()
    for k in range(3):
        r.launch("SPCBPT_eye", 0, rows=(8 * k, 48, 3))
    np.testing.assert_array_equal(r.read_accum(), whole)


def test_full_size_properties(gpu, pkg, ob):
    """BASELINE config 2 size (Cornell 1024x1024): properties that need no oracle run — accumulation is the running
    mean (idempotent for a repeated frame), every pixel written, SPCBPT and PT means agree."""
    scene = pkg.scenes.cornell_box()
    r = pkg.Renderer(scene, 0)
    cam = scene.camera
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], 1.0)
    r.resize(1024, 1024)
    r.set_light_trace(100000, 52, 1)
    r.set_subspace()   # minimal valid tuple computed by the library
    for f in range(8):
        r.launch("pt", f)
    pt = r.read_accum()
    assert (pt[..., 3] == 1.0).all() and np.isfinite(pt).all()
    r.clear_accum()
    for f in range(8):
        r.render_frame("SPCBPT_eye", f)
    sp = r.read_accum()
    assert (sp[..., 3] == 1.0).all() and np.isfinite(sp).all()
    assert abs(sp[..., :3].mean() - pt[..., :3].mean()) / pt[..., :3].mean() < 0.01
    # lerp(prev, cur, 1/(n+1)) with cur == prev's sample leaves a converged pixel unchanged: rerender frame 0 twice
    r.clear_accum()
    r.launch("pt", 0); a = r.read_accum().copy()
    r.launch("pt", 0); b = r.read_accum()
    np.testing.assert_array_equal(a, b)


def test_error_behaviour(gpu, pkg):
    scene = pkg.scenes.cornell_box()
    r = pkg.Renderer(scene, 0)
    with pytest.raises(pkg.SpcbptError):
        r.launch("pt", 0)                      # before resize / camera
    r.set_camera_lookat((0, 1, 5), (0, 1, 0), (0, 1, 0), 35.0, 1.0)
    r.resize(16, 16)
    with pytest.raises(pkg.SpcbptError):
        r.launch("SPCBPT_eye", 0)              # no sampler yet
    with pytest.raises(pkg.SpcbptError):
        r.launch("no such alg", 0)
    with pytest.raises(pkg.SpcbptError):
        r.launch("pt", 0, rows=(3, 16, 1))     # row_begin must be a band boundary
    r.launch("pt", 0)
    r.sync()


# ---- the HBM part of the traversal stack -----------------------------------------------------------------------------------
def _needle_rays(n, seed=5):
    rng = np.random.default_rng(seed)
    return _rays(rng, n, np.array([-0.9, 0.1, -0.9]), np.array([0.9, 1.85, 0.9]))


def test_deep_traversal_stack_spills_to_hbm_and_matches_oracle(gpu, pkg, ob):
    """TravStack keeps 16 entries per lane in LDS and spills deeper ones to HBM (csrc/device_lib.h).  Furniture scenes hardly
    ever go past 16; a cloud of room-spanning slivers (scenes.needle_room) makes sibling boxes overlap at every level, so a ray
    enters nearly every child and the stack runs to ~3 x depth.  Same bar as the other traversal cases (same triangle for
    >= 99.9 % of rays, |dt| <= 1e-5), plus proof that the spill area was written."""
    scene = pkg.scenes.needle_room(20000)
    r, o = _pair(pkg, ob, scene, 8, 8)
    info = r.scene_info()
    assert 3 * info["bvh_depth"] - 16 > 0, info
    rays = _needle_rays(20000)
    r.trace_closest(rays[:256])            # sizes the spill area of the light stream
    r.spill_arm()
    t1, tri1, uv1 = r.trace_closest(rays)
    written, entries = r.spill_count()
    assert entries == 3 * info["bvh_depth"] - 16 and written > 1000, (written, entries)
    t0, tri0, uv0 = o.trace_closest(rays)
    same = tri0 == tri1
    assert same.mean() >= 0.999, same.mean()
    # slivers are hit at all angles and their Moller-Trumbore determinant is tiny, so the distance depends on the evaluation order:
    # the kernel contracts its cross products to FMAs and multiplies by v_rcp_f32(det), the oracle rounds every product and
    # divides.  Measured: 94.7 % of the rays within 1e-5, max 2.7e-4 -- the bar here is 90 % / 1e-3 for every ray; the furniture
    # scenes of test_traversal_matches_oracle_bvh keep 1e-5 for ALL rays with the same code
    err = np.abs(t0 - t1)[same] / np.maximum(1.0, t0[same])
    assert (err <= 1e-5).mean() >= 0.9 and err.max() <= 1e-3, ((err <= 1e-5).mean(), err.max())
    rays2 = _needle_rays(20000, seed=6)
    rays2[:, 7] = np.random.default_rng(7).uniform(0.05, 2.0, len(rays2))
    r.spill_arm()
    v1 = r.trace_any(rays2)
    assert r.spill_count()[0] > 0
    assert (o.trace_any(rays2) == v1).mean() >= 0.999


def test_traversal_stack_overflow_is_reported_not_silent(gpu, pkg, monkeypatch):
    """A spill area that is too small (only reachable with the developer cap SPCBPT_DEBUG_SPILL_ENTRIES) loses subtrees; the
    next synchronising call must say so instead of returning wrong hits."""
    scene = pkg.scenes.needle_room(20000)
    monkeypatch.setenv("SPCBPT_DEBUG_SPILL_ENTRIES", "1")
    r = pkg.Renderer(scene, 0)
    monkeypatch.delenv("SPCBPT_DEBUG_SPILL_ENTRIES")
    with pytest.raises(pkg.SpcbptError, match="traversal stack overflow"):
        r.trace_closest(_needle_rays(4000))
    r.sync()                                        # the report is one-shot: the context stays usable
    cam = scene.camera
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], 1.0)
    r.resize(32, 32)
    r.launch("pt", 0)
    with pytest.raises(pkg.SpcbptError, match="traversal stack overflow"):
        r.sync()


def test_batched_eye_launch_sizes_its_spill_area_for_the_grid_it_launches(gpu, pkg, ob):
    """A batch of 4 frames of a small image launches up to 4x the blocks of one frame; every block indexes the spill area by its
    own block id.  (Round-1 bug: the area was sized for one frame's blocks, the other blocks wrote past its end whenever one
    frame's share was below the resident grid.)  Deep-stack scene, 160 x 120: batched == frame by frame, bit for bit, the spill
    path in use, and the image agrees with the oracle."""
    import os
    scene = pkg.scenes.needle_room(20000)
    cam = scene.camera
    W, H, NF = 160, 120, 4

    def make(batch):
        if batch > 1:
            os.environ["SPCBPT_EYE_BATCH"] = str(batch)
        try:
            r = pkg.Renderer(scene, 0)
        finally:
            os.environ.pop("SPCBPT_EYE_BATCH", None)
        r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
        r.resize(W, H)
        r.set_light_trace(4000, 64, 1)
        return r

    a = make(1)
    o = ob.Oracle(scene)
    o.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
    o.resize(W, H); o.set_light_trace(4000, 64, 1)
    tup = minimal_tuple(o, 2)
    a.set_subspace(*tup); o.set_subspace(*tup); o.set_cmf_double(True)
    for f in range(NF):
        a.launch("light trace", f + 1); a.build_sampler(); a.launch("SPCBPT_eye", f)
    a.sync()
    want = a.read_accum().copy()
    b = make(NF)
    b.set_subspace(*tup)
    for f in range(NF):
        b.launch("light trace", f + 1); b.build_sampler()
    b.launch_eye_batch([0])                # allocates this stream's spill area ... for ONE frame's grid
    b.sync(); b.clear_accum()
    for f in range(NF):
        b.launch("light trace", f + 1); b.build_sampler()
    b.spill_arm()
    b.launch_eye_batch(list(range(NF)))
    b.sync()
    assert b.spill_count()[0] > 0
    assert np.array_equal(b.read_accum(), want)
    for f in range(NF):
        o.launch("light trace", f + 1); o.build_sampler(); o.launch("SPCBPT_eye", f)
    # against the oracle only the image mean: thousands of 2-6 mm slivers put a path's every second ray within rounding of an
    # edge, where two different BVHs legitimately pick different triangles, so per-pixel agreement is not a property of this
    # scene (57 % of pixels within 2e-3 at equal seeds); 77 k samples give the mean to a few percent
    s = image_parity(want[..., :3], o.read_accum()[..., :3])
    assert s["mean_rel"] < 0.06, s


# ---- label caching (csrc/device_lib.h) ---------------------------------------------------------------------------------------
def test_cached_vertex_labels_are_the_labels_the_reference_derives(gpu, pkg, ob):
    """The timed kernels classify a vertex once under both trees and carry the labels (EyeVertex::lsub, light vertex `pad` = eye-tree
    label + 1); the counting kernels re-derive them per connection / RMIS update as rmis.h does.  Same labels -> same image (the two
    instantiations may contract FMAs differently: >= 99.9 % of pixels within 2e-3, not bit equality); the labels stored in the
    cache are checked against the oracle's tree_index one by one; a classifier WITH direction nodes makes labels direction-dependent
    and must take the generic kernels (image parity with the oracle; the batched launch, which only exists cached, refuses)."""
    from tests.parity_util import grid_tree_tuple
    scene = pkg.scenes.bedroom(target_tris=40000, tex_size=64)
    r, o = _pair(pkg, ob, scene, 96, 64, lt=(4000, 64, 1))
    tup = grid_tree_tuple(pkg, o, scene)
    r.set_subspace(*tup); o.set_subspace(*tup); o.set_cmf_double(True)
    for f in range(3):
        r.render_frame("SPCBPT_eye", f)
    cached = r.read_accum()[..., :3].copy()
    lvc = r.lvc_read()
    surf = lvc["depth"] > 0
    assert (lvc["pad"][surf] > 0).all() and (lvc["pad"][~surf] == 0).all()
    d = np.zeros((surf.sum(), 3), np.float32)                       # direction is irrelevant: no direction nodes in these trees
    want = ob.tree_index(tup[0], np.concatenate([lvc["position"][surf], lvc["normal"][surf], d], 1))
    assert np.array_equal(lvc["pad"][surf].astype(np.int64) - 1, want)
    r.clear_accum(); r.enable_counters(True)
    for f in range(3):
        r.render_frame("SPCBPT_eye", f)
    generic = r.read_accum()[..., :3].copy()
    r.enable_counters(False)
    assert (r.lvc_read()["pad"] == 0).all()                          # the reference-order light pass does not fill the cache field
    s = image_parity(cached, generic)
    assert s["frac_close"] >= 0.999 and s["mean_rel"] < 1e-4 and tails_explained(s), s
    # mixed: a cache traced WITHOUT labels (pad = 0) rendered by the caching eye kernel -> it descends per connection
    r.clear_accum()
    for f in range(3):
        r.enable_counters(True); r.launch("light trace", f + 1); r.enable_counters(False)
        r.build_sampler(); r.launch("SPCBPT_eye", f)
    s = image_parity(r.read_accum()[..., :3], cached)
    assert s["frac_close"] >= 0.999 and tails_explained(s), s
    # a classifier with a direction node on top: labels depend on the viewing direction
    et, lt, q, g = tup
    def with_direction_root(t):
        n = len(t)
        t2 = np.zeros(n + 1, dtype=t.dtype)
        t2[1:] = t
        t2["child"][1:] = np.where(t["leaf"][:, None] == 1, t["child"], t["child"] + 1)
        t2[0]["type"] = 2; t2[0]["mid"] = (0.0, 0.0, 0.0); t2[0]["leaf"] = 0
        t2[0]["child"] = [1, 1, 1, 1, n, n, n, n]                   # +z-facing directions -> a different leaf (the last node)
        return t2
    assert et[-1]["leaf"] == 1
    et2, lt2 = with_direction_root(et), with_direction_root(lt)
    r.set_subspace(et2, lt2, q, g); o.set_subspace(et2, lt2, q, g)
    r.clear_accum(); o.clear_accum()
    for f in range(2):
        r.render_frame("SPCBPT_eye", f); o.render_frame("SPCBPT_eye", f)
    s = image_parity(r.read_accum()[..., :3], o.read_accum()[..., :3])
    assert s["frac_close"] >= 0.997 and s["mean_rel"] < 1e-2 and tails_explained(s), s
    with pytest.raises(pkg.SpcbptError, match="direction"):
        r.launch_eye_batch([0])


@pytest.mark.parametrize("lt,shard", [((4000, 52, 1), (700, 1900)), ((60, 400, 50), (0, 60))])   # lane-per-path / the reference's kind: many paths per core
def test_batched_light_passes_leave_the_caches_of_single_passes(gpu, pkg, monkeypatch, lt, shard):
    """spcbpt_launch_light_batch: n light passes as one persistent launch whose core queue spans the frames.  Every pass must leave
    the cache (vertices in (core, slot) order, vertex and path counts), the sampler tables and finally the image that the n single
    "light trace" launches leave -- bit for bit, for a shard of the cores (core_begin > 0) and a batch that wraps around the ring
    of buffer sets."""
    import torch
    scene = pkg.scenes.cornell_box()
    cam = scene.camera
    W, H, NF = 96, 96, 5
    monkeypatch.setenv("SPCBPT_EYE_BATCH", str(NF))
    monkeypatch.setenv("SPCBPT_SETS", "7")          # 5 sets per batch in a ring of 7: the second batch wraps
    r = pkg.Renderer(scene, 0)
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
    r.resize(W, H)
    r.set_light_trace(*lt, core_begin=shard[0], core_count=shard[1])
    r.set_subspace()
    with pytest.raises(pkg.SpcbptError, match="light_ahead"):
        r.launch_light_batch(1, NF)                  # the passes must queue up
    dev = torch.device("cuda", 0)

    def cache_of_oldest_pass():
        r.sync_light()
        dv, dc, cap = r.lvc_export()
        n, paths = pkg.dist.device_view(dc, 8, dev).view(torch.int32).cpu().numpy()
        v = pkg.dist.device_view(dv, int(n) * 96, dev).cpu().numpy().view(pkg.api.LIGHT_VERTEX_DTYPE).copy()
        return int(n), int(paths), v

    want = []
    for rnd in range(2):
        for f in range(NF):
            r.launch("light trace", 10 * rnd + f + 1)
            n, paths, v = cache_of_oldest_pass()
            r.build_sampler()
            want.append((n, paths, v, r.sampler_read()))
        r.launch_eye_batch([NF * rnd + f for f in range(NF)])
    r.sync()
    img = r.read_accum().copy()
    assert all(w[0] > w[1] and w[1] == shard[1] * lt[2] for w in want)
    r.clear_accum()
    r.set_light_ahead(True)
    k = 0
    for rnd in range(2):
        r.launch_light_batch(10 * rnd + 1, NF)
        for f in range(NF):
            n, paths, v = cache_of_oldest_pass()
            wn, wp, wv, ws = want[k]; k += 1
            assert (n, paths) == (wn, wp)
            assert v.tobytes() == wv.tobytes()
            r.build_sampler()
            sub, cmfs, jump, vc, pc = r.sampler_read()
            assert (vc, pc) == (ws[3], ws[4])
            assert np.array_equal(sub, ws[0]) and np.array_equal(cmfs, ws[1]) and np.array_equal(jump, ws[2])
        r.launch_eye_batch([NF * rnd + f for f in range(NF)])
    r.sync()
    assert np.array_equal(r.read_accum(), img)
    with pytest.raises(pkg.SpcbptError):
        r.launch_light_batch(1, 33)


def test_counting_sampler_build_gives_the_tables_of_the_radix_sort(gpu, pkg, monkeypatch):
    """The four-launch sampler build (one stable counting sort over the subspace ids) against the hipcub form it replaces, on a
    bedroom-class cache with hundreds of occupied subspaces: jump buffer, ranges and counts identical, CMFs to double rounding."""
    scene = pkg.scenes.bedroom(target_tris=40000)
    cam = scene.camera
    out = {}
    tup = None
    for form in ("hipcub", "counting"):
        monkeypatch.setenv("SPCBPT_SAMPLER_BUILD", form)
        r = pkg.Renderer(scene, 0)
        r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], 4 / 3)
        r.resize(64, 48)
        r.set_light_trace(20000, 52, 1)
        if tup is None:
            r.preprocess(200_000, 200_000, False)      # many-leaf trees, initial Gamma
            tup = r.get_subspace()
        else:
            r.set_subspace(*tup)
        r.launch("light trace", 5); r.build_sampler()
        out[form] = r.sampler_read()
        # and through the path that refills the keys (an imported cache)
        lvc = r.lvc_read()
        r.lvc_import(lvc); r.build_sampler()
        again = r.sampler_read()
        assert np.array_equal(again[2], out[form][2]) and np.array_equal(again[0], out[form][0]) and again[3:] == out[form][3:]
    a, b = out["hipcub"], out["counting"]
    assert a[3:] == b[3:] and a[3] > 40000
    assert (a[0]["size"] > 0).sum() > 100
    np.testing.assert_array_equal(a[0]["size"], b[0]["size"])
    np.testing.assert_array_equal(a[0]["jump_bias"], b[0]["jump_bias"])
    np.testing.assert_array_equal(a[2], b[2])
    np.testing.assert_allclose(a[1], b[1], rtol=0, atol=1.5e-7)
    np.testing.assert_allclose(a[0]["sum_pmf"], b[0]["sum_pmf"], rtol=1e-6)


def test_a_batch_of_twenty_frames_equals_twenty_launches(gpu, pkg, monkeypatch):
    """Frame ids beyond 15 (the id of a published eye vertex travels in 6 bits since launches hold up to 32 frames): 20 light passes
    in one launch, 20 frames in one eye launch, against 20 x (light pass, build, eye launch) -- the same film bit for bit."""
    scene = pkg.scenes.cornell_box()
    cam = scene.camera
    W, H, NF = 64, 64, 20
    def make(batch):
        monkeypatch.setenv("SPCBPT_EYE_BATCH", str(batch))
        monkeypatch.setenv("SPCBPT_RENDER_STREAMS", "1")
        r = pkg.Renderer(scene, 0)
        r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
        r.resize(W, H)
        r.set_light_trace(3000, 52, 1)
        r.set_subspace()
        return r
    a = make(1)
    for f in range(NF):
        a.launch("light trace", f + 1); a.build_sampler(); a.launch("SPCBPT_eye", f)
    a.sync()
    want = a.read_accum().copy()
    b = make(NF)
    b.set_light_ahead(True)
    b.launch_light_batch(1, NF)
    for f in range(NF):
        b.build_sampler()
    b.launch_eye_batch(list(range(NF)))
    b.sync()
    assert np.array_equal(b.read_accum(), want)
    with pytest.raises(pkg.SpcbptError):
        b.launch_eye_batch(list(range(33)))


def test_batched_sampler_build_and_merge_equal_single_ones(gpu, pkg, monkeypatch):
    """spcbpt_build_sampler_batch builds the samplers of n queued light passes with the kernels of one build (frame = the grid's second
    dimension), and a batched eye launch merges its frames into the film in one pass: tables and film must be those of n single
    builds and n single merges, bit for bit -- on a many-subspace tuple, with subframe indices that restart in mid-batch (a merge
    that must NOT read the film) and with a second batch that wraps around the ring of buffer sets."""
    scene = pkg.scenes.bedroom(target_tris=40000)
    cam = scene.camera
    W, H, NF = 128, 72, 5
    monkeypatch.setenv("SPCBPT_EYE_BATCH", str(NF))
    monkeypatch.setenv("SPCBPT_SETS", "7")
    r = pkg.Renderer(scene, 0)
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
    r.resize(W, H)
    r.set_light_trace(6000, 52, 1)
    r.preprocess(200_000, 200_000, False)      # many-leaf trees, initial Gamma
    r.set_light_ahead(True)
    subframes = [[0, 1, 2, 3, 4], [5, 0, 1, 2, 3]]     # the second batch restarts the running mean at its second frame

    def run(batched):
        r.clear_accum()
        tabs = []
        for rnd in range(2):
            r.launch_light_batch(10 * rnd + 1, NF)
            if batched:
                r.build_sampler_batch(NF)
            else:
                for f in range(NF):
                    r.build_sampler()
            tabs.append(r.sampler_read())          # the set built last
            r.launch_eye_batch(subframes[rnd])
        r.sync()
        return tabs, r.read_accum().copy(), r.read_frame().copy()

    t1, a1, f1 = run(False)
    t2, a2, f2 = run(True)
    for x, y in zip(t1, t2):
        assert (x[3], x[4]) == (y[3], y[4]) and x[3] > 1000
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and np.array_equal(x[2], y[2])
    assert np.isfinite(a1).all() and np.array_equal(a1, a2) and np.array_equal(f1, f2)
    # frame by frame: the same film as single launches with single merges
    r.clear_accum()
    for rnd in range(2):
        r.launch_light_batch(10 * rnd + 1, NF)
        for f in range(NF):
            r.build_sampler()
            r.launch("SPCBPT_eye", subframes[rnd][f])
    r.sync()
    assert np.array_equal(r.read_accum(), a2) and np.array_equal(r.read_frame(), f2)
    with pytest.raises(pkg.SpcbptError):
        r.build_sampler_batch(33)
    with pytest.raises(pkg.SpcbptError):
        r.build_sampler_batch(0)


@pytest.mark.gpu
def test_batched_build_scratch_is_sized_by_the_batch_and_falls_back_when_it_cannot_be_had(gpu, pkg, monkeypatch):
    """The scratch of spcbpt_build_sampler_batch is n frames x the largest item bound of the builds at hand x 16 B (+ histograms) --
    not 32 frames x the padded capacity; it is freed by spcbpt_lvc_set_capacity and by leaving light-ahead mode; and when the device
    refuses it (SPCBPT_DEBUG_BATCH_SCRATCH_LIMIT) the batch is built one pass at a time with the SAME tables."""
    scene = pkg.scenes.cornell_box()
    cam = scene.camera
    monkeypatch.setenv("SPCBPT_EYE_BATCH", "8")
    r = pkg.Renderer(scene, 0)
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], 1.0)
    r.resize(64, 64)
    r.set_light_trace(3000, 64, 1)
    r.set_subspace()
    r.set_light_ahead(True)
    assert r.batch_scratch() == {"bytes": 0, "frames": 0, "fallbacks": 0}
    r.launch_light_batch(1, 3)
    r.build_sampler_batch(3)
    cap, _ = r.lvc_capacity()
    st = r.batch_scratch()
    assert st["frames"] == 3 and st["fallbacks"] == 0          # 3, not the 8 (or 32) the context is sized for
    assert 3 * cap * 16 <= st["bytes"] <= 3 * (cap + 4096) * 16 + 3 * (4 << 20)   # + the per-frame block histograms
    want = r.sampler_read()
    r.launch_eye_batch([0, 1, 2]); r.sync()
    film = r.read_accum().copy()
    # freed with the capacity it was sized for, and when passes stop running ahead
    r.lvc_set_capacity(cap)
    assert r.batch_scratch()["bytes"] == 0
    r.launch_light_batch(1, 3); r.build_sampler_batch(3)
    assert r.batch_scratch()["bytes"] > 0
    r.launch_eye_batch([0, 1, 2]); r.sync()
    r.set_light_ahead(False)
    assert r.batch_scratch()["bytes"] == 0
    # the device "refuses": single builds, same tables, same film
    r.set_light_ahead(True)
    monkeypatch.setenv("SPCBPT_DEBUG_BATCH_SCRATCH_LIMIT", "4096")
    r.clear_accum()
    r.launch_light_batch(1, 3)
    r.build_sampler_batch(3)
    st = r.batch_scratch()
    assert st["bytes"] == 0 and st["fallbacks"] == 1
    got = r.sampler_read()
    assert (got[3], got[4]) == (want[3], want[4])
    assert all(np.array_equal(x, y) for x, y in zip(got[:3], want[:3]))
    r.launch_eye_batch([0, 1, 2]); r.sync()
    assert np.array_equal(r.read_accum(), film)
    # a refused size is remembered (no device-wide wait and four hipMallocs per call), until the mode or the capacity changes
    monkeypatch.delenv("SPCBPT_DEBUG_BATCH_SCRATCH_LIMIT")
    r.launch_light_batch(1, 3); r.build_sampler_batch(3)
    assert r.batch_scratch() == {"bytes": 0, "frames": 0, "fallbacks": 2}
    r.launch_eye_batch([0, 1, 2]); r.sync()
    r.set_light_ahead(False); r.set_light_ahead(True)
    r.launch_light_batch(1, 2); r.build_sampler_batch(2)
    small = r.batch_scratch()
    assert small["frames"] == 2 and small["bytes"] > 0 and small["fallbacks"] == 2
    r.launch_eye_batch([0, 1]); r.sync()
    # a grow attempt that fails keeps the scratch that exists: the next 2-frame batch still runs batched
    monkeypatch.setenv("SPCBPT_DEBUG_BATCH_SCRATCH_LIMIT", "4096")
    r.launch_light_batch(1, 3); r.build_sampler_batch(3)
    assert r.batch_scratch() == {"bytes": small["bytes"], "frames": 2, "fallbacks": 3}
    r.launch_eye_batch([0, 1, 2]); r.sync()
    r.launch_light_batch(1, 2); r.build_sampler_batch(2)
    assert r.batch_scratch() == {"bytes": small["bytes"], "frames": 2, "fallbacks": 3}


@pytest.mark.gpu
def test_a_cache_the_device_cannot_hold_leaves_an_empty_consistent_context(gpu, pkg, ob, monkeypatch):
    """Round 6 (advisor): if an allocation of the buffer-set ring fails half-way, the context is left WITHOUT a cache and says so --
    not with half of its sets allocated and the old pointers freed.  The refusal is simulated (SPCBPT_DEBUG_LVC_LIMIT); afterwards a
    capacity the device can hold works, and the frames are the frames of a context that never saw the failure."""
    scene = pkg.scenes.cornell_box()
    r, o = _pair(pkg, ob, scene, 64, 64)
    r2, _ = _pair(pkg, ob, scene, 64, 64)
    for x in (r, r2):
        x.set_subspace()
    r.launch("light trace", 1); r.build_sampler(); r.launch("SPCBPT_eye", 0); r.sync()
    cap, sets = r.lvc_capacity()
    assert cap > 0 and sets > 0
    monkeypatch.setenv("SPCBPT_DEBUG_LVC_LIMIT", str(cap))
    with pytest.raises(pkg.SpcbptError, match="NO cache"):
        r.lvc_set_capacity(4 * cap)
    assert r.lvc_capacity()[0] == 0                                   # empty, not half-allocated
    with pytest.raises(pkg.SpcbptError):                                # nothing renders from a cache that is not there
        r.build_sampler()
    monkeypatch.delenv("SPCBPT_DEBUG_LVC_LIMIT")
    r.lvc_set_capacity(cap)                                             # a size the device can hold: the context works again
    assert r.lvc_capacity()[0] == cap
    for x in (r, r2):
        x.clear_accum()
        for f in range(2):
            x.render_frame("SPCBPT_eye", f, launch_frame=50 + f)
        x.sync()
    assert np.array_equal(r.read_accum(), r2.read_accum())
