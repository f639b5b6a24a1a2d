"""Kernel time (spcbpt_kernel_time("lt")) of the light-tracing estimator in its two modes -- float atomics against records + radix sort
+ ordered gather (spcbpt_set_splat_order) -- at 1920 x 1080 on the bench scene with 100 000 light paths, both in the same run: two
passes of 30 launches each, every launch behind a light pass and a sampler build of its own.  The ordered mode is timed twice: as a
host loop queues it (no wait since the light pass, so the launch runs over the cache's capacity, about twice the vertex count) and
with a sync in front of the launch (the light pass has left its count in pinned memory: the launch runs over the count).
(DESIGN.md 8b).  usage: python tools/splat_order_cost.py [tris]"""
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
r.set_light_trace(100000, 52, 1)
r.set_subspace()
MODES = (("atomic", pkg.api.SPLAT_ATOMIC, False), ("ordered", pkg.api.SPLAT_ORDERED, False), ("ordered, count known", pkg.api.SPLAT_ORDERED, True))


def frame(f, wait):
    r.launch("light trace", f + 1)
    r.build_sampler()
    if wait:
        r.sync()
    r.launch("lt", f)
    r.sync()


for name, mode, wait in MODES:           # warm-up: allocations, first launches
    r.set_splat_order(mode)
    for f in range(4):
        frame(f, wait)
vertices = len(r.read_splat_records()[1])
print(f"cache: {vertices} vertices, capacity {r.lvc_capacity()[0]}", flush=True)
r.enable_kernel_timing(True)
for p in range(2):
    out = []
    for name, mode, wait in MODES:
        r.set_splat_order(mode)
        frame(0, wait)                   # (the buffers of the ordered mode come back with the mode)
        frame(1, wait)
        r.reset_kernel_time()
        for i in range(30):
            frame(4 + 30 * p + i, wait)
        out.append("%s %.4f ms (%d launches)" % ((name,) + r.kernel_time("lt")))
    print(f"pass {p}: " + "; ".join(out), flush=True)
