"""Kernel times (spcbpt_kernel_time) of the reflected-guide pass at 1920 x 1080 next to the first-hit feature pass of the same frame, on
the bench scene and on scenes.mirror_box(), with the default parameters: 4 warm-up frames, then 5 passes of 20 launches each; the
median pass and the spread (min .. max) of the per-launch means.  usage: python tools/guides_cost.py [tris]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g   # noqa: E402

pkg = g.load_package()
W, H = 1920, 1080
for scene in (pkg.scenes.bedroom(target_tris=int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000), pkg.scenes.mirror_box()):
    r = pkg.Renderer(scene, 0)
    cam = scene.camera
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
    r.resize(W, H)
    for f in range(4):                       # warm-up: allocations, first launches
        r.launch_features(f)
        r.launch_guides(f)
    r.sync()
    r.enable_kernel_timing(True)
    per = {"features": [], "guides": []}
    for p in range(5):
        r.reset_kernel_time()
        for i in range(20):
            f = 4 + 20 * p + i
            r.launch_features(f)
            r.launch_guides(f)
            r.sync()
        for name in per:
            per[name].append(r.kernel_time(name)[0])   # the average per launch of this pass
    print(f"{scene.name} ({len(scene.indices)} triangles): " + ", ".join(
        "%s median %.4f ms (%.4f .. %.4f over 5 passes of 20)" % (name, statistics.median(v), min(v), max(v)) for name, v in per.items()), flush=True)
    del r
