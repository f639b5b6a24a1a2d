"""Row f4, eye side: escaped eye sub-paths that see the environment map (spcbpt_set_environment_mode, SPCBPT_ENV_EYE_SEES_SKY) and
"pt"'s sky shadow ray along the sampled direction (SPCBPT_ENV_PT_SKY_SHADOW_ALONG_DIR), on the GPU.

Upstream's __miss__BDPTVertex only ends an eye sub-path that leaves the scene, so rmis::light_hit_env has no caller although the
recursive-MIS weights of the other sky strategies count it: "SPCBPT_eye" is biased dark and directly seen sky is black.
The oracle's test knobs (set_env_miss_strategy / set_pt_env_nee_fixed) complete the estimator; the device's opt-in mode restates
them (eye_walk.h: eye_sky_miss, the k_spcbpt_sky kernels).  The default stays upstream's: tests/test_gpu_env.py is unchanged."""
import os
import subprocess

import numpy as np
import pytest

from tests.parity_util import image_parity, tails_explained

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 96, 64
CAM = dict(eye=(0.0, 2.6, 2.6), lookat=(0.0, 0.2, 0.0), up=(0, 1, 0), fov=40.0)
UP_CAM = dict(eye=(0.0, 2.0, 0.0), lookat=(0.0, 10.0, 0.0), up=(0, 0, -1), fov=40.0)   # above the walls, looking out of the open top
LT = (6000, 64, 1)
SKY_MISS = 8                      # SPCBPT_UNIT_SKY_MISS
ERR_INVALID_ARG, ERR_STATE = -1, -5


@pytest.fixture(scope="module")
def yard(gpu, pkg, ob):
    """The courtyard with its sky and a trained tuple, on the device and in the oracle (as tests/test_gpu_env.py)."""
    scene = pkg.scenes.courtyard()
    env = scene.environment
    r = pkg.Renderer(scene, 0)
    o = ob.Oracle(scene)
    for x in (r, o):
        x.set_camera_lookat(CAM["eye"], CAM["lookat"], CAM["up"], CAM["fov"], W / H)
        x.resize(W, H)
        x.set_environment(env["rgba"], env["center"], env["radius"])
        x.set_light_trace(*LT)
    r.set_pretrace(20000, 10)
    r.preprocess(target_paths=100000, target_q_paths=100000, train=True)
    tup = r.get_subspace()
    o.set_subspace(*tup)
    o.set_cmf_double(True)
    return dict(scene=scene, r=r, o=o, tup=tup)


def _renderer(pkg, scene, cam=CAM, mode=1, tup=None, batch=None):
    if batch:
        os.environ["SPCBPT_EYE_BATCH"] = str(batch)
    try:
        r = pkg.Renderer(scene, 0)
    finally:
        os.environ.pop("SPCBPT_EYE_BATCH", None)
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
    r.resize(W, H)
    if scene.environment is not None:
        env = scene.environment
        r.set_environment(env["rgba"], env["center"], env["radius"])
    r.set_light_trace(*LT)
    if tup is None:
        r.set_subspace()
    else:
        r.set_subspace(*tup)
    r.set_environment_mode(mode)
    return r


def _sky_miss(r, ev, w):
    n = len(ev)
    words = np.zeros((n, 32), np.uint32)
    words[:, :25] = np.ascontiguousarray(ev).view(np.uint32).reshape(n, 25)
    words[:, 25:28] = np.float32(1.0).view(np.uint32)           # NextVertex.flux, singlePdf: the weight does not depend on them
    words[:, 28] = np.float32(1.0).view(np.uint32)
    words[:, 29:32] = np.ascontiguousarray(w, dtype=np.float32).view(np.uint32)
    out = r.unit(SKY_MISS, words, 6)
    return out[:, :3].view(np.float32), out[:, 3].view(np.float32), out[:, 4].astype(np.int64)


def test_sky_miss_weight_is_the_balance_heuristic(yard):
    """The device's SKY_MISS weight of camera paths that leave the scene after D surface vertices equals the weight computed from
    nothing but the vertices' pdfs (orc_debug_env_partition), and with the device's own CONNECT weights of the same path's other
    strategies it sums to 1 -- which upstream's sign of the flux multiplier (miss weight 0.03 where 0.99 is right) would fail."""
    from tests.test_gpu_first_principles import _weights
    r, o = yard["r"], yard["o"]
    for depth in (1, 2, 3):
        wo, truth, ev, lv = o.env_partition(depth, 600, vertices=True)
        assert len(wo) >= 150, (depth, len(wo))
        ok = np.abs(wo[:, 0] - 1) < 1e-3
        assert ok.mean() > 0.99
        truth, ev, lv = truth[ok], ev[ok], lv[ok]
        w_esc = -lv[:, 0]["normal"]                              # y0 = the sky direction: its normal is minus the direction to the sky (orc_debug_env_partition)
        rgb, got, label = _sky_miss(r, ev[:, 0], w_esc)
        assert (label == lv[:, 0]["subspace_id"]).mean() > 0.99   # SKY.getLabel of the escape direction (a cell border may flip one)
        assert np.isfinite(rgb).all() and (rgb >= 0).all()
        d = np.abs(got - truth[:, 0])
        print("sky miss", depth, np.percentile(d, [50, 99.5, 100]))
        assert np.percentile(d, 99.5) < 2e-4 and d.max() < 5e-3, (depth, np.percentile(d, [50, 99.5, 100]))
        total = got.astype(np.float64)
        for k in range(min(depth, 4)):
            total += _weights(r, ev[:, k], lv[:, k])
        assert np.percentile(np.abs(total - 1), 99.5) < 5e-4, (depth, np.percentile(np.abs(total - 1), [50, 99.5, 100]))


def test_images_with_the_sky_seen_match_the_oracle_knobs(yard):
    """"SPCBPT_eye" with SPCBPT_ENV_EYE_SEES_SKY against the oracle's env_miss_strategy, "pt" with SPCBPT_ENV_PT_SKY_SHADOW_ALONG_DIR
    against its pt_env_nee_fixed: the bars of tests/test_gpu_env.py."""
    r, o = yard["r"], yard["o"]
    try:
        r.set_environment_mode(1); o.set_env_miss_strategy(True)
        r.clear_accum(); o.clear_accum()
        for f in range(4):
            r.render_frame("SPCBPT_eye", f); o.render_frame("SPCBPT_eye", f)
        a, b = r.read_accum(), o.read_accum()
        assert (a[..., 3] == 1.0).all()
        s = image_parity(a[..., :3], b[..., :3])
        assert s["frac_close"] >= 0.998 and s["mean_rel"] < 1e-2 and tails_explained(s), s
        r.set_environment_mode(2); o.set_env_miss_strategy(False); o.set_pt_env_nee_fixed(True)
        r.clear_accum(); o.clear_accum()
        for f in range(4):
            r.launch("pt", f); o.launch("pt", f)
        s = image_parity(r.read_accum()[..., :3], o.read_accum()[..., :3])
        assert s["frac_close"] >= 0.998 and s["mean_rel"] < 1e-2 and tails_explained(s), s
    finally:
        r.set_environment_mode(0); o.set_env_miss_strategy(False); o.set_pt_env_nee_fixed(False)


def _batch_means(r, alg, frames, batches):
    """Image means of `batches` consecutive batches of frames / batches frames each, from the running mean of one film."""
    per = frames // batches
    r.clear_accum()
    cum, means = 0.0, []
    for b in range(batches):
        for f in range(b * per, (b + 1) * per):
            r.render_frame(alg, f)
        m = float(r.read_accum()[..., :3].astype(np.float64).mean())
        means.append(m * (b + 1) * per - cum)
        cum = m * (b + 1) * per
    return np.asarray(means) / per


def test_spcbpt_with_the_sky_seen_converges_to_pt(yard, pkg):
    """The completed estimator: the image mean of "SPCBPT_eye" with SPCBPT_ENV_EYE_SEES_SKY is that of "pt" with
    SPCBPT_ENV_PT_SKY_SHADOW_ALONG_DIR within 1.5 %; without the strategy it is far darker (the missing strategy's MIS share, and
    the directly seen sky).  FRAMES spp in BATCHES batches; the test also checks its own power: 1.5 % must be at least 4 sigma
    of the ratio, sigma from the batch-to-batch spread of both estimators.  Measured once on MI355X: sigma 0.28 % (0.43 % at 512
    spp in 8 batches, too little for the bar), ratio 0.9998, the mean without the strategy 0.37 of the mean with it."""
    FRAMES, BATCHES = 2048, 16
    r = _renderer(pkg, yard["scene"], tup=yard["tup"], mode=1)
    sp1 = _batch_means(r, "SPCBPT_eye", FRAMES, BATCHES)
    r.set_environment_mode(2)
    pt2 = _batch_means(r, "pt", FRAMES, BATCHES)
    r.set_environment_mode(0)
    sp0 = _batch_means(r, "SPCBPT_eye", FRAMES // 4, 2)
    rel_sigma = np.sqrt((sp1.std(ddof=1) / sp1.mean()) ** 2 + (pt2.std(ddof=1) / pt2.mean()) ** 2) / np.sqrt(BATCHES)
    ratio = sp1.mean() / pt2.mean()
    print("SPCBPT(sky seen) / pt(along dir)", ratio, "sigma", rel_sigma, "without the strategy", sp0.mean() / sp1.mean())
    assert 4 * rel_sigma <= 0.015, rel_sigma
    assert abs(ratio - 1) < 0.015, (ratio, rel_sigma)
    assert sp0.mean() < 0.8 * sp1.mean(), (sp0.mean(), sp1.mean())


def test_directly_seen_sky(yard, pkg):
    """Every primary ray leaves the scene: with the strategy the SPCBPT film is pt's (both draw the same camera_ray, the weight of
    an eye depth of 1 is 1, only pdf_G / pdf_G rounding differs); without it the film is black, as upstream's."""
    scene = yard["scene"]
    r = _renderer(pkg, scene, cam=UP_CAM, mode=1)
    for f in range(2):
        r.render_frame("SPCBPT_eye", f)
    sp = r.read_accum()[..., :3].copy()
    r.clear_accum()
    for f in range(2):
        r.launch("pt", f)
    pt = r.read_accum()[..., :3].copy()
    assert (pt > 0).any(axis=-1).all()                                   # the sky everywhere
    np.testing.assert_allclose(sp, pt, rtol=1e-6, atol=0)
    r.set_environment_mode(0)
    r.clear_accum()
    for f in range(2):
        r.render_frame("SPCBPT_eye", f)
    assert (r.read_accum()[..., :3] == 0).all()


def test_every_launch_form_renders_the_sky_strategy(yard, pkg):
    """With SPCBPT_ENV_EYE_SEES_SKY: the batched eye launch, a deferred launch + merge, and the sharded host loop of two ranks on
    one GPU give the films of plain frame-by-frame launches bit for bit (as tests/test_gpu_pipeline.py for the default mode)."""
    import torch
    scene = yard["scene"]
    NF = 4
    plain = _renderer(pkg, scene)
    for f in range(NF):
        plain.render_frame("SPCBPT_eye", f)
    plain.sync()
    want = plain.read_accum().copy()
    # the directly seen sky is in it, and the film differs from the default mode's
    base = _renderer(pkg, scene, mode=0)
    for f in range(NF):
        base.render_frame("SPCBPT_eye", f)
    assert want[..., :3].mean() > 1.1 * base.read_accum()[..., :3].mean()
    # batched
    b = _renderer(pkg, scene, batch=4)
    for f in range(NF):
        b.launch("light trace", f + 1); b.build_sampler()
    b.launch_eye_batch(list(range(NF)))
    b.sync()
    assert np.array_equal(b.read_accum(), want)
    # deferred + merge
    d = _renderer(pkg, scene)
    for f in range(NF):
        d.launch("light trace", f + 1); d.build_sampler()
        d.launch_deferred("SPCBPT_eye", f)
        d.merge_deferred(True)
    d.sync()
    assert np.array_equal(d.read_accum(), want)
    # two ranks on one GPU, the sharded host loop (interleaved bands, gathered caches, batched eye launches)
    dev = torch.device("cuda", 0)
    M, WORLD, BATCH = LT[0], 2, 2
    VB = pkg.dist.VERTEX_BYTES
    tup = plain.get_subspace()
    ranks = []
    for k in range(WORLD):
        r = _renderer(pkg, scene, batch=BATCH, tup=tup)
        lo, cnt = pkg.dist.core_range(M, k, WORLD)
        r.set_light_trace(M, LT[1], LT[2], core_begin=lo, core_count=cnt)
        r.set_light_ahead(True)
        r.launch("light trace", 1)
        ranks.append(r)
    stage = [[None, None] for _ in range(WORLD)]
    queued = []
    for f in range(NF):
        shards = []
        for r in ranks:
            r.launch("light trace", f + 2)
            dv, dc, cap = r.lvc_export()
            r.sync_light()
            n = int(pkg.dist.device_view(dc, 8, dev).view(torch.int32)[0].item())
            shards.append(pkg.dist.device_view(dv, n * VB, dev))
        gathered = torch.cat(shards)
        total = gathered.numel() // VB
        torch.cuda.current_stream(dev).synchronize()
        for k, r in enumerate(ranks):
            r.lvc_import_wait()
            stage[k][f & 1] = gathered.clone()
            torch.cuda.current_stream(dev).synchronize()
            r.lvc_import_device(stage[k][f & 1].data_ptr(), total)
            r.build_sampler()
        queued.append(f)
        if len(queued) == BATCH:
            for k, r in enumerate(ranks):
                r.launch_eye_batch(queued, pkg.dist.band_rows(H, k, WORLD))
            queued = []
    for r in ranks:
        r.sync()
    films = [r.read_accum() for r in ranks]
    assert np.array_equal(films[0] + films[1], want)


def test_environment_mode_api(yard, pkg):
    r = _renderer(pkg, yard["scene"], mode=0)
    lib, h = r.lib, r.h
    assert lib.spcbpt_set_environment_mode(h, 4) == ERR_INVALID_ARG
    assert lib.spcbpt_set_environment_mode(h, -1) == ERR_INVALID_ARG
    for flags in (3, 1, 2, 0):
        r.set_environment_mode(flags)
        assert r.environment()["flags"] == flags
    # not while a deferred frame is outstanding; the flags stay
    r.set_environment_mode(1)
    r.launch("light trace", 1); r.build_sampler()
    r.launch_deferred("SPCBPT_eye", 0)
    assert lib.spcbpt_set_environment_mode(h, 0) == ERR_STATE
    r.merge_deferred(True)
    assert r.environment()["flags"] == 1
    # the counting kernels know no sky strategy: refused, not rendered without it
    r.enable_counters(True)
    r.launch("light trace", 2); r.build_sampler()
    assert lib.spcbpt_launch(h, b"SPCBPT_eye", 1, 0, H, 1) == ERR_STATE
    r.set_environment_mode(0)
    r.launch("SPCBPT_eye", 1)
    r.enable_counters(False)
    r.sync()
    # a context without a sky renders bit-identically whatever the flags (set before any sky would be)
    cb = pkg.scenes.cornell_box()
    films = []
    for flags in (0, 3):
        c = _renderer(pkg, cb, cam=cb.camera, mode=flags)
        for f in range(2):
            c.render_frame("SPCBPT_eye", f)
        for f in range(2):
            c.launch("pt", f + 2)
        c.sync()
        films.append(c.read_accum())
    assert np.array_equal(films[0], films[1])


def test_render_tool_installs_the_scene_sky(yard, pkg, tmp_path):
    """tools/spcbpt_render on a .scene that names an env_file, "SPCBPT_eye" with --env-mode 1: the PFM it writes is the film of
    the same frame sequence driven through ctypes on the same loaded scene."""
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "spcbpt_render"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    path = pkg.scenes.write_scene(pkg.scenes.courtyard(), str(tmp_path), "yard")
    assert "env_file" in open(path).read()
    w, h, frames = 64, 48, 3
    out = str(tmp_path / "tool")
    r = subprocess.run([os.path.join(ROOT, "tools", "spcbpt_render"), path, str(tmp_path), "--alg", "SPCBPT_eye", "--minimal", "--env-mode", "1",
                        f"--dim={w}x{h}", "--frames", str(frames), "--out", out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "environment map" in r.stdout, r.stdout
    raw = open(out + ".pfm", "rb").read()
    head = raw.split(b"\n", 3)
    assert head[0] == b"PF" and head[1] == f"{w} {h}".encode()
    tool = np.frombuffer(head[3], np.float32).reshape(h, w, 3)            # bottom row first = the accum orientation
    s2, warn = pkg.load_scene_file(path, str(tmp_path))
    assert s2.environment is not None
    c = pkg.Renderer(s2, 0)
    cam = s2.camera
    c.set_environment(s2.environment["rgba"], s2.environment["center"], s2.environment["radius"])
    c.set_environment_mode(1)
    c.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
    c.resize(w, h)
    c.set_light_trace(100000, 52, 1, 0, 0, True)                           # the tool's light pass
    c.set_subspace()
    for f in range(frames):
        c.launch("light trace", 1000001 + f); c.build_sampler(); c.launch("SPCBPT_eye", f)
    c.sync()
    film = c.read_accum()[..., :3]
    assert film.mean() > 0
    assert np.array_equal(tool, film)
