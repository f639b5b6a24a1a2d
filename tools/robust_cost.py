"""The bucket film and the robust resolve, measured.
  python tools/robust_cost.py cost    kernel times (spcbpt_kernel_time) at 1920 x 1080 on the Cornell box (the new kernels are image-space
      passes: the scene does not enter), "pt" with the moments and K = 8, 16, 32 buckets on, two passes each: the spans "buckets" and
      "robust_resolve" next to "moments" and "film_merge" of the same run.  Every launch is followed by a sync.
  python tools/robust_cost.py equal   equal samples on the Cornell box under the sphere lamp (256 x 256, minimal tuple): 32 and 128 frames of
      "pt" and of "SPCBPT_eye", RMSE and relative RMSE of accum and of the robust image (K = 8 and 16, strength 0.5 / 1 / 2) against a
      2048-frame film of the same algorithm."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g   # noqa: E402

pkg = g.load_package()


def spans(r, names):
    return ", ".join("%s %.4f ms (%d)" % ((n,) + r.kernel_time(n)) for n in names)


def cost():
    scene = pkg.scenes.cornell_box()
    cam = scene.camera
    W, H = 1920, 1080
    r = pkg.Renderer(scene, 0)
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
    r.resize(W, H)
    r.set_film_moments(True)
    for K in (8, 16, 32):
        r.set_film_buckets(K)
        for f in range(K + 2):               # warm-up: allocations, first launches, every bucket live
            r.launch("pt", f)
        r.robust_resolve(1.0)
        r.sync()
        r.enable_kernel_timing(True)
        f = K + 2
        for p in range(2):
            r.reset_kernel_time()
            for _ in range(20):
                r.launch("pt", f)
                r.robust_resolve(1.0)
                r.sync()
                f += 1
            w = r.read_robust()[0][..., 3]
            print(f"K = {K}, pass {p}: " + spans(r, ("pt", "moments", "buckets", "film_merge", "robust_resolve")) + f"; buckets kept: mean {w.mean():.2f}, min {w.min():.0f}", flush=True)
        r.reset_kernel_time()
        for _ in range(4):
            r.launch("pt", 0)                # subframe 0 rewrites all K planes
            r.sync()
        print(f"K = {K}, subframe 0 (restart, writes all K planes): " + spans(r, ("buckets",)), flush=True)
        r.enable_kernel_timing(False)


def equal():
    scene = pkg.scenes.cornell_sphere_lamp()
    W = H = 256
    cam = scene.camera

    def ctx(K):
        r = pkg.Renderer(scene, 0)
        r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
        r.resize(W, H)
        r.set_light_trace(100000, 52, 1)
        r.set_subspace()
        r.set_film_buckets(K)
        return r

    def frame(r, alg, f):
        if alg == "SPCBPT_eye":
            r.launch("light trace", f + 1)
            r.build_sampler()
        r.launch(alg, f)

    for alg in ("pt", "SPCBPT_eye"):
        ref_ctx = ctx(0)
        for f in range(2048):
            frame(ref_ctx, alg, f)
        ref = ref_ctx.read_accum()[..., :3].astype(np.float64)
        rmse = lambda a: float(np.sqrt(np.mean((a[..., :3].astype(np.float64) - ref) ** 2)))
        rel = lambda a: float(np.sqrt(np.mean(((a[..., :3].astype(np.float64) - ref) / (ref + 1e-2)) ** 2)))
        bias = lambda a: float(np.mean(a[..., :3].astype(np.float64) - ref) / np.mean(ref))
        print(f"cornell_sphere_lamp {W}x{H}, {alg}; reference: 2048 frames (it shares the first samples of every run below: at most 128 of 2048)", flush=True)
        for K in (8, 16):
            r = ctx(K)
            for f in range(128):
                frame(r, alg, f)
                if f + 1 in (32, 128):
                    a = r.read_accum()
                    print(f"  {f + 1} frames, K = {K}: accum RMSE {rmse(a):.5f}, relative RMSE {rel(a):.5f}", flush=True)
                    for s in (0.5, 1.0, 2.0):
                        r.robust_resolve(s)
                        o = r.read_robust()[0]
                        print(f"      strength {s}: robust RMSE {rmse(o):.5f}, relative RMSE {rel(o):.5f}, mean difference {100 * bias(o):+.2f} % of the mean "
                              f"(accum {100 * bias(a):+.2f} %), buckets kept: mean {o[..., 3].mean():.2f} of {min(K, f + 1)}", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "equal":
        equal()
    else:
        cost()
