"""The display transform, measured.
  python tools/display_cost.py [tris]   kernel times (spcbpt_kernel_time) at 1920 x 1080 on a 16-frame "pt" film of the bedroom-class
      scene (default 200 000 triangles: the pass is image-space, the scene only supplies the film's luminance distribution), the moments
      on: the spans "display_hist" (memset + histogram + exposure kernel) and "display" (the tone map), manual and auto, every operator,
      two passes of 20 calls each, every call followed by a sync -- next to "moments" and "film_merge" of the film's own 16 launches, the
      measuring stick: each reads the same 33 MB once.  Also the histogram's occupancy (bins in use, the fullest bin's share): the
      LDS adds of a wave serialise where its lanes meet in one bin."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g   # noqa: E402

pkg = g.load_package()


def spans(r, names):
    return ", ".join("%s %.4f ms (%d)" % ((n,) + r.kernel_time(n)) for n in names)


def main():
    tris = int(sys.argv[1]) if len(sys.argv) > 1 else 200_000
    scene = pkg.scenes.bedroom(target_tris=tris, tex_size=256)
    cam = scene.camera
    W, H, FRAMES = 1920, 1080, 16
    r = pkg.Renderer(scene, 0)
    r.set_camera_lookat(cam["eye"], cam["lookat"], cam["up"], cam["fov"], W / H)
    r.resize(W, H)
    r.set_film_moments(True)
    r.launch("pt", 0)                        # warm-up: allocations, first launches
    r.display("film", auto=True)
    r.display("film")
    r.sync()
    r.enable_kernel_timing(True)
    r.reset_kernel_time()
    for f in range(FRAMES):
        r.launch("pt", f)
        r.sync()
    print(f"bedroom ({tris} triangles) {W}x{H}, {FRAMES} frames of pt: " + spans(r, ("pt", "moments", "film_merge")), flush=True)
    for op in ("film", "reinhard", "aces", "linear"):
        for label, kw in (("manual EV 0", dict(ev=0.0)), ("manual + histogram", dict(ev=0.0, histogram=True)), ("auto", dict(auto=True))):
            for p in range(2):
                r.reset_kernel_time()
                for _ in range(20):
                    r.display("film", op=op, **kw)
                    r.sync()
                names = ("display",) if label == "manual EV 0" else ("display_hist", "display")
                print(f"{op}, {label}, pass {p}: " + spans(r, names), flush=True)
    r.enable_kernel_timing(False)
    r.display("film", auto=True)
    out8, ev = r.read_display()
    hist = r.read_display_histogram().astype(np.int64)
    inr = hist[:256]
    print(f"auto EV {ev:.4f}; histogram: {int((inr > 0).sum())} of 256 bins in use, fullest bin {inr.max() / hist.sum():.3%} of the pixels, "
          f"top 8 bins {np.sort(inr)[-8:].sum() / hist.sum():.3%}, dark {hist[256] / hist.sum():.3%}, bright {hist[257] / hist.sum():.3%}; "
          f"mean byte of the display plane {out8[..., :3].mean():.1f}, of read_frame {r.read_frame()[..., :3].mean():.1f}", flush=True)


if __name__ == "__main__":
    main()
