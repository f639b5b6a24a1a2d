"""Kernel times (spcbpt_kernel_time) of the history passes with and without the variance they can carry, and of the history denoiser
next to "denoise_variance", at 1920 x 1080 on the bench scene: per setting of the moments switch two passes of 30 camera moves each
(capture, an orbit of 2 degrees there or back, one frame, its features, reproject, resolve and -- moments on -- a 5-iteration
history denoise and a 5-iteration denoise_variance).  usage: python tools/history_denoise_cost.py [tris]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g   # noqa: E402

pkg = g.load_package()
scene = pkg.scenes.bedroom(target_tris=int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000)
cam = scene.camera
W, H = 1920, 1080
d = np.asarray(cam["eye"], np.float64) - np.asarray(cam["lookat"], np.float64)
a = np.radians(2.0)
eyes = (np.asarray(cam["eye"], np.float64),
        np.asarray(cam["lookat"], np.float64) + np.array([d[0] * np.cos(a) + d[2] * np.sin(a), d[1], -d[0] * np.sin(a) + d[2] * np.cos(a)]))

for moments in (False, True):
    r = pkg.Renderer(scene, 0)
    r.set_camera_lookat(eyes[0], cam["lookat"], cam["up"], cam["fov"], W / H)
    r.resize(W, H)
    r.set_film_moments(moments)

    def move(i):
        r.history_capture(1)
        r.set_camera_lookat(eyes[i & 1], cam["lookat"], cam["up"], cam["fov"], W / H)
        r.launch("pt", 0)
        r.launch_features(0)
        r.history_reproject()
        r.history_resolve(1)
        if moments:
            r.history_denoise(5)
            r.denoise_variance(5)

    r.launch("pt", 0)
    r.launch_features(0)
    for i in range(1, 4):                    # warm-up: allocations, first launches
        move(i)
    r.sync()
    r.enable_kernel_timing(True)
    spans = ("pt", "features", "moments", "history_capture", "reproject", "resolve") + (("history_denoise", "denoise_variance") if moments else ())
    for p in range(2):
        r.reset_kernel_time()
        for i in range(30):
            move(i)
            r.sync()
        live = float((r.read_history(False, False, True)["prior"][..., 3] > 0).mean())
        print(f"moments {'on' if moments else 'off'}, pass {p}: " + ", ".join("%s %.4f ms (%d launches)" % ((name,) + r.kernel_time(name)) for name in spans) +
              f"; {100 * live:.1f} % of the pixels carry history", flush=True)
    r.close()
