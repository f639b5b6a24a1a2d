"""The batched merge that keeps the moments and the buckets, measured.
  python tools/merge_stats_cost.py kernel [tris]   kernel times (spcbpt_kernel_time, every launch followed by a sync) at 1920 x 1080 on the
      bench scene (bedroom, 1 000 000 triangles unless given; minimal tuple -- the merges are image-space passes), 100 000 light paths:
      per frame "moments" + "buckets" + "film_merge" of 20 spcbpt_launch("SPCBPT_eye") calls against ONE "film_merge_stats" of a 20-frame
      spcbpt_launch_eye_batch_film, with the moments alone and with K = 8 buckets beside them; three passes each after a warm-up pass.
  python tools/merge_stats_cost.py loop [tris] [frames]   the whole loop: tools/spcbpt_render on the bench scene (written as glTF),
      --target-error 1e-9 --check-every 20 over `frames` (default 200) frames with the trained tuple, without --batch, with --batch 20
      and with --batch 20 on one render stream, each twice: the tool's own seconds for the frames (preprocessing excluded) as
      milliseconds per frame, and whether all runs wrote the same bytes."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g   # noqa: E402

pkg = g.load_package()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N = 1920, 1080, 20


def kernel(tris):
    scene = pkg.scenes.bedroom(target_tris=tris)
    cam = scene.camera
    os.environ["SPCBPT_EYE_BATCH"] = str(N)
    os.environ["SPCBPT_RENDER_STREAMS"] = "1"
    r = pkg.Renderer(scene, 0)
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
    r.resize(W, H)
    r.set_light_trace(100000, 52, 1)
    r.set_subspace()
    r.enable_kernel_timing(True)
    light = 1
    for K in (0, 8):
        r.set_film_moments(True)
        r.set_film_buckets(K)
        names = ("moments", "buckets", "film_merge") if K else ("moments", "film_merge")
        r.clear_accum()
        f = 0
        for p in range(4):   # pass 0 warms up: allocations, first launches, every bucket live
            r.reset_kernel_time()
            for _ in range(N):
                r.render_frame("SPCBPT_eye", f, launch_frame=light)
                r.sync()
                f += 1; light += 1
            t = {n: r.kernel_time(n) for n in names}
            total = sum(v[0] for v in t.values())
            print(f"K = {K}, per frame, pass {p}: " + ", ".join(f"{n} {v[0]:.4f} ms ({v[1]})" for n, v in t.items()) +
                  f"; sum {total:.4f} ms per frame, {N * total:.3f} ms per {N} frames", flush=True)
        r.clear_accum()
        r.set_light_ahead(True)
        f = 0
        for p in range(4):
            r.reset_kernel_time()
            r.launch_light_batch(light, N); light += N
            r.build_sampler_batch(N)
            r.launch_eye_batch_film(list(range(f, f + N)))
            r.sync()
            f += N
            ms, count = r.kernel_time("film_merge_stats")
            eye, _ = r.kernel_time("spcbpt_render")
            print(f"K = {K}, batched, pass {p}: film_merge_stats {ms:.4f} ms ({count}) per {N} frames, {ms / N:.4f} ms per frame; eye kernel {eye:.3f} ms per {N} frames", flush=True)
        r.set_light_ahead(False)
    r.enable_kernel_timing(False)


def loop(tris, frames):
    tool = os.path.join(ROOT, "tools", "spcbpt_render")
    p = subprocess.run(["make", "-C", os.path.join(ROOT, "tools"), "spcbpt_render"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-3000:]
    with tempfile.TemporaryDirectory() as tmp:
        path = pkg.scenes.write_gltf(pkg.scenes.bedroom(target_tris=tris), tmp, "bedroom", binary=True)
        files = []
        one = {"SPCBPT_RENDER_STREAMS": "1"}   # what bench.py runs its batched loop with (the library's default is two render streams)
        runs = [("plain", [], {}), ("batch20", ["--batch", str(N)], {}), ("batch20, one render stream", ["--batch", str(N)], one)]
        for name, extra, env in runs + [(n + " again", x, e) for n, x, e in runs]:
            out = os.path.join(tmp, name.replace(" ", "_").replace(",", ""))
            cmd = [tool, path, tmp, "--alg", "SPCBPT_eye", f"--dim={W}x{H}", "--frames", str(frames), "--target-error", "1e-9", "--check-every", str(N),
                   "--out", out] + extra
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600, env=dict(os.environ, **env))
            assert p.returncode == 0, p.stdout[-3000:]
            m = re.search(r"(\d+) subframes of SPCBPT_eye at \d+x\d+: ([0-9.]+) s", p.stdout)
            e = re.search(r"(\d+) frames used, error reached (\S+)", p.stdout)
            sec, n = float(m.group(2)), int(m.group(1))
            print(f"{name}: {n} frames in {sec:.3f} s, {1e3 * sec / n:.3f} ms per frame; error reached {e.group(2)}", flush=True)
            files.append(open(out + ".pfm", "rb").read())
        print(f"the {len(files)} runs wrote the same .pfm bytes:", all(f == files[0] for f in files), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    tris = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    if mode == "loop":
        loop(tris, int(sys.argv[3]) if len(sys.argv) > 3 else 200)
    else:
        kernel(tris)
