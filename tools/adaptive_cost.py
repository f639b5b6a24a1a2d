"""Adaptive sampling, measured.
  python tools/adaptive_cost.py cost [tris]   kernel times (spcbpt_kernel_time) at 1920 x 1080 on the bench scene, trained tuple, two passes each:
      the ordinary single-frame "SPCBPT_eye" launch with the moments on (spans spcbpt_render, moments, film_merge), adaptive_select
      (k_tile_error + k_tile_select), and adaptive_eye / adaptive_merge with 100, 50, 25 and 10 % of the tiles listed -- every k-th
      tile, and one contiguous run of tiles.  Every launch is followed by a sync, so no span overlaps the next light pass.
  python tools/adaptive_cost.py equal         equal work on the Cornell box under the sphere lamp (256 x 256, minimal tuple): uniform N frames
      against adaptive runs that stop at the same number of tile-samples, RMSE against a 2048-frame render."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g   # noqa: E402

pkg = g.load_package()


def spans(r, names):
    return ", ".join("%s %.4f ms (%d)" % ((n,) + r.kernel_time(n)) for n in names)


def cost(tris):
    scene = pkg.scenes.bedroom(target_tris=tris)
    r = pkg.Renderer(scene, 0)
    cam = scene.camera
    W, H = 1920, 1080
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
    r.resize(W, H)
    r.set_light_trace(100000, 52, 1)
    r.preprocess(target_paths=2_000_000, target_q_paths=2_000_000, train=True)
    r.set_film_moments(True)
    frame = [0]

    def uniform():
        r.launch("light trace", 1000 + frame[0])
        r.build_sampler()
        r.launch("SPCBPT_eye", frame[0])
        r.sync()
        frame[0] += 1

    for _ in range(4):
        uniform()
    r.enable_kernel_timing(True)
    for p in range(2):
        r.reset_kernel_time()
        for _ in range(12):
            uniform()
        print(f"uniform pass {p}: " + spans(r, ("spcbpt_render", "moments", "film_merge")), flush=True)
    r.adaptive_begin(frame[0])
    st = r.adaptive_state()
    n_tiles = st["tiles_x"] * st["tiles_y"]
    err = None
    for p in range(2):
        r.reset_kernel_time()
        for _ in range(20):
            n = r.adaptive_select(0.05, 4, 0)
        print(f"select pass {p}: {n} of {n_tiles} tiles above 0.05; " + spans(r, ("adaptive_select",)), flush=True)
    err = r.read_adaptive()["error"]
    print("tile error after %d frames: median %.4f, 90 %% %.4f, max %.4f" % (frame[0], np.median(err), np.quantile(err, 0.9), err.max()), flush=True)
    lf = [5000]
    for layout in ("every k-th tile", "one contiguous run"):
        for pct in (100, 50, 25, 10):
            k = 100 // pct
            count = n_tiles // k
            tiles = np.arange(0, n_tiles, k) if layout[0] == "e" else np.arange(min(n_tiles // 3, n_tiles - count), min(n_tiles // 3, n_tiles - count) + count)
            r.adaptive_set_tiles(tiles)
            for p in range(3):      # pass 0 warms the shape up
                r.reset_kernel_time()
                for _ in range(8):
                    lf[0] += 1
                    r.launch("light trace", lf[0])
                    r.build_sampler()
                    r.launch_adaptive()
                    r.sync()
                if p:
                    print(f"{layout}, {pct} % ({tiles.size} tiles), pass {p - 1}: " + spans(r, ("adaptive_eye", "adaptive_merge")), flush=True)
    s = r.read_adaptive()["samples"]
    print("counts after the runs: %d .. %d; checksum %.6f" % (s.min(), s.max(), float(np.float64(r.read_accum()[..., :3]).sum())))


def equal():
    scene = pkg.scenes.cornell_sphere_lamp()
    W = H = 256
    cam = scene.camera

    def ctx():
        r = pkg.Renderer(scene, 0)
        r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
        r.resize(W, H)
        r.set_light_trace(100000, 52, 1)
        r.set_subspace()
        r.set_film_moments(True)
        return r

    def uniform(r, f):
        r.launch("light trace", f + 1)
        r.build_sampler()
        r.launch("SPCBPT_eye", f)

    ref_ctx = ctx()
    for f in range(2048):
        uniform(ref_ctx, f)
    ref = ref_ctx.read_accum()[..., :3].astype(np.float64)
    rmse = lambda a: float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - ref) ** 2)))
    rel = lambda a: float(np.sqrt(np.mean(((a[..., :3].astype(np.float64) - ref) / (ref + 1e-2)) ** 2)))
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    print(f"cornell_sphere_lamp {W}x{H}, {tiles} tiles; reference: 2048 uniform frames (it shares the first samples of every run below: at most 64 of 2048)")
    for N in (16, 32):
        u = ctx()
        for f in range(N):
            uniform(u, f)
        a = u.read_accum()
        u.adaptive_begin(N)
        u.adaptive_select(0.0)
        e = u.read_adaptive()["error"]
        print(f"uniform {N} frames: {tiles * N} tile-samples, RMSE {rmse(a):.5f}, relative RMSE {rel(a):.5f}; tile error median {np.median(e):.4f}, max {e.max():.4f}", flush=True)
        for frac in (1.0, 0.5):
            target = frac * float(np.median(e))
            r = ctx()
            for f in range(4):
                uniform(r, f)
            r.adaptive_begin(4)
            used, rounds = tiles * 4, 0
            while True:
                n = r.adaptive_select(target, 4, 256)
                if n == 0 or used + n > tiles * N:
                    break
                rounds += 1
                r.launch("light trace", 5 + rounds)
                r.build_sampler()
                r.launch_adaptive()
                used += n
            s = r.read_adaptive()["samples"]
            a = r.read_accum()
            print(f"  adaptive, target {target:.4f} ({frac} x that median), min 4, max 256: {used} tile-samples ({100.0 * used / (tiles * N):.1f} % of uniform {N}) in {rounds} launches, "
                  f"counts {s.min()} .. {s.max()}, last selection {n} tiles: RMSE {rmse(a):.5f}, relative RMSE {rel(a):.5f}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "equal":
        equal()
    else:
        cost(int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000)
