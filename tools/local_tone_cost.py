"""The local tone stage, measured.  Image-space: two seeded HDR images of 1920 x 1080 -- ROOM: twelve stops of
large-scale range under two stops of per-pixel noise, with 64 small emitters, the kind of image the stage is for; NOISE: per-pixel
log-uniform luminance over twenty stops, where about two thirds of the bins of every node column are active -- through spcbpt_display_image,
spcbpt_bloom_image and spcbpt_local_tone_image, five warm-up calls and twenty timed ones each, every call followed by a sync.
  python tools/local_tone_cost.py spans       the kernel-time spans (HIP events on the stream): "display_hist" and "display" of an auto
      display call, "bloom" with its defaults at six levels, "local_tone" with the defaults and with cell 8, range 0.5, blur 4, on both
      images, alternating orders, two passes
  python tools/local_tone_cost.py profile     the workload alone, for a kernel trace:
      rocprofv3 --kernel-trace --stats -d <dir> -- python tools/local_tone_cost.py profile      (no counters in the same run)
  python tools/local_tone_cost.py report <dir>  per kernel of that trace: launches per call, mean and least time
  python tools/local_tone_cost.py effect      scenes.cornell_sphere_lamp, "pt", 512 x 512, 256 frames: the share of pixels with a channel
      at 255 and the share with every channel below 8, of the film and of the local tone plane at the film's auto exposure"""
import csv
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H, WARM, CALLS = 1920, 1080, 5, 20
SETS = (("defaults (cell 16, range 1, blur 1)", dict()), ("cell 8, range 0.5, blur 4", dict(cell=8, range=0.5, blur=4)))
IMAGES = ("room", "noise")


def image(kind="room"):
    rng = np.random.default_rng(8)
    img = np.ones((H, W, 4), np.float32)
    if kind == "noise":
        img[..., :3] = (2.0 ** rng.uniform(-10.0, 10.0, (H, W, 1)) * rng.uniform(0.2, 1.0, (H, W, 3))).astype(np.float32)
        return img
    yy, xx = np.mgrid[0:H, 0:W]
    room = 2.0 ** (6.0 * np.sin(xx / 300.0) * np.cos(yy / 200.0) - 2.0)               # twelve stops of large-scale range
    img[..., :3] = (room[..., None] * 2.0 ** rng.uniform(-1.0, 1.0, (H, W, 1)) * rng.uniform(0.2, 1.0, (H, W, 3))).astype(np.float32)
    img[rng.integers(0, H, 64), rng.integers(0, W, 64), :3] *= 4096.0                 # small emitters far above the key
    return img


def renderer():
    import __graft_entry__ as g
    pkg = g.load_package()
    return pkg, pkg.Renderer(pkg.scenes.cornell_box(), 0)


def spans(r, names):
    return ", ".join("%s %.4f ms (%d)" % ((n,) + r.kernel_time(n)) for n in names)


def run_spans():
    pkg, r = renderer()
    imgs = {k: image(k) for k in IMAGES}
    img = imgs["room"]
    cases = [(k, label, kw) for k in IMAGES for label, kw in SETS]
    for k, _, kw in cases:
        for _ in range(WARM):
            r.local_tone_image(imgs[k], **kw)
            r.sync()
    for _ in range(WARM):
        r.bloom_image(img, levels=6)
        r.display_image(img, auto=True)
        r.sync()
    r.enable_kernel_timing(True)
    for p in range(2):
        r.reset_kernel_time()
        for _ in range(CALLS):
            r.display_image(img, auto=True)
            r.sync()
        print(f"{W}x{H} display_image, auto, pass {p}: " + spans(r, ("display_hist", "display")), flush=True)
        r.reset_kernel_time()
        for _ in range(CALLS):
            r.bloom_image(img, levels=6)
            r.sync()
        print(f"{W}x{H} bloom_image, L = 6, pass {p}: " + spans(r, ("bloom",)), flush=True)
        for k, label, kw in (cases if p == 0 else cases[::-1]):
            r.reset_kernel_time()
            for _ in range(CALLS):
                r.local_tone_image(imgs[k], **kw)
                r.sync()
            print(f"{W}x{H} local_tone_image, {k}, {label}, pass {p}: " + spans(r, ("local_tone",)), flush=True)
    r.enable_kernel_timing(False)
    for k, label, kw in cases:
        r.local_tone_image(imgs[k], **kw)
        print(f"{k}, {label}: equal to local_tone_host:", r.read_local_tone().tobytes() == pkg.api.local_tone_host(imgs[k], **kw).tobytes(), flush=True)


def run_profile():
    _, r = renderer()
    for k in IMAGES:
        img = image(k)
        for _, kw in SETS:
            for _ in range(WARM + CALLS):
                r.local_tone_image(img, **kw)
                r.sync()


def report(d):
    rows = []   # the trace as rocprofv3 left it: *kernel_trace.csv (--output-format csv) or its database (the view `kernels`)
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    for f in glob.glob(os.path.join(d, "**", "*_results.db"), recursive=True):
        import sqlite3
        for name, start, end, grid in sqlite3.connect(f).execute("select name, start, end, grid_x from kernels"):
            rows.append({"Kernel_Name": name, "Start_Timestamp": start, "End_Timestamp": end, "Grid_Size_X": grid})
    if not rows:
        sys.exit(f"no *kernel_trace.csv and no *_results.db under {d}")
    rows = [r for r in rows if "k_lt_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = []   # a call starts at its k_lt_build
    for r in rows:
        name = r["Kernel_Name"].replace("void ", "").replace("spc::", "").split("(")[0]
        if "k_lt_build" in name:
            calls.append([])
        calls[-1].append((name, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    per = WARM + CALLS
    labels = [f"{k}, {label}" for k in IMAGES for label, _ in SETS]
    print(f"{W}x{H}: kernel trace of {per} local_tone_image calls per image and parameter set ({len(calls)} calls found); the last {CALLS} calls of each")
    for g, label in enumerate(labels):
        group = calls[g * per:(g + 1) * per][-CALLS:]
        if not group:
            break
        print(f"  {label}: {len(group[0])} launches per call")
        agg = {}
        for call in group:
            for name, us in call:
                agg.setdefault(name, []).append(us)
        total = 0.0
        for name, v in agg.items():
            n = len(v) / len(group)
            total += sum(v) / len(group)
            print(f"    {name:24s} {n:4.1f} per call  mean {sum(v) / len(v):8.2f} us  min {min(v):8.2f} us")
        print(f"    sum of the mean times per call: {total:.2f} us")


def run_effect():
    pkg, _ = renderer()
    scene = pkg.scenes.cornell_sphere_lamp()
    w = h = 512
    cam = scene.camera
    r = pkg.Renderer(scene, 0)
    U, V, Wv = pkg.camera_frame(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
    r.set_camera(np.array(cam["eye"], np.float32), U, V, Wv)
    r.resize(w, h)
    r.set_light_trace(20000, 16, 1)
    for f in range(256):
        r.launch("pt", f)
    r.display("film", auto=True)
    film8, ev = r.read_display()

    lit = (r.read_accum()[..., :3] > 0).any(-1)      # the camera stands outside the room: the pixels beside its opening hold zeros and keep them

    def shares(img8):
        rgb = img8[..., :3][lit]
        return 100.0 * float((rgb == 255).any(-1).mean()), 100.0 * float((rgb < 8).all(-1).mean())
    print(f"cornell_sphere_lamp {w}x{h}, pt, 256 frames, tone film, auto exposure EV {ev:.3f}; {100.0 * lit.mean():.2f} % of the pixels hold light, the shares are of those")
    print("  the film:                         %.2f %% of the pixels with a channel at 255, %.2f %% with every channel below 8" % shares(film8))
    for c in (0.5, 0.3):
        r.local_tone("film", compress=c)
        r.display("local", ev=ev)
        print("  local tone, compress %.1f, same EV: %.2f %% of the pixels with a channel at 255, %.2f %% with every channel below 8" % ((c,) + shares(r.read_display()[0])))
    lum = r.read_accum()[..., :3] @ np.float32([0.3, 0.6, 0.1])
    lt = r.read_local_tone()[..., :3] @ np.float32([0.3, 0.6, 0.1])
    ok = lum > 0
    print("  log2 luminance, 1st to 99th percentile: the film %.2f stops, the local tone plane (compress 0.3) %.2f stops" % (
        np.subtract(*np.percentile(np.log2(lum[ok]), (99, 1))), np.subtract(*np.percentile(np.log2(lt[ok]), (99, 1)))))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "spans"
    if mode == "spans":
        run_spans()
    elif mode == "profile":
        run_profile()
    elif mode == "report":
        report(sys.argv[2])
    elif mode == "effect":
        run_effect()
    else:
        sys.exit(__doc__)
