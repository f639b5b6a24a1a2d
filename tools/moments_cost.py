"""Kernel times (spcbpt_kernel_time) of the film's moment update, the film error and the variance-guided denoiser at 1920 x 1080 on the
bench scene, next to "pt" and the plain "denoise" span from the same run: two passes of 30 launches each, 5 a-trous iterations
(DESIGN.md 8e).  usage: python tools/moments_cost.py [tris]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g   # noqa: E402

pkg = g.load_package()
scene = pkg.scenes.bedroom(target_tris=int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000)
r = pkg.Renderer(scene, 0)
cam = scene.camera
W, H = 1920, 1080
r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
r.resize(W, H)
r.set_film_moments(True)
for f in range(4):                       # warm-up: allocations, first launches
    r.launch("pt", f)
    r.launch_features(f)
r.denoise(5)
r.denoise_variance(5)
r.film_error()
r.sync()
r.enable_kernel_timing(True)
SPANS = ("pt", "moments", "film_error", "denoise", "denoise_variance")
for p in range(2):
    r.reset_kernel_time()
    for i in range(30):
        f = 4 + 30 * p + i
        r.launch("pt", f)
        r.launch_features(f)
        r.denoise(5)
        r.denoise_variance(5)
        e = r.film_error()
        r.sync()
    print(f"pass {p}: " + ", ".join("%s %.4f ms (%d launches)" % ((name,) + r.kernel_time(name)) for name in SPANS) + f"; film error {e['mean']:.4f}", flush=True)
