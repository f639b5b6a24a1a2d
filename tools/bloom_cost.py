"""The bloom stage, measured.  Image-space only: a seeded HDR image of 1920 x 1080 through spcbpt_display_image and
spcbpt_bloom_image, L = 6, five warm-up calls and twenty timed ones each, every call followed by a sync.
  python tools/bloom_cost.py spans            the kernel-time spans (HIP events on the stream): "display_hist" and "display" of an auto
      display call, "bloom" with the fused coarse tail cut at two levels and with per-level kernels only (SPCBPT_BLOOM_TAIL), two
      alternating passes each
  python tools/bloom_cost.py profile          the workload alone, for a kernel trace:
      rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bloom_cost.py profile      (no counters in the same run)
  python tools/bloom_cost.py report <dir>     per kernel and grid size of that trace: launches per call, mean time, the bytes the kernel
      must move (computed from the level sizes) and the bandwidth that implies, next to k_display_map and k_display_histogram of the
      same run"""
import csv
import glob
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, H, LEVELS, WARM, CALLS = 1920, 1080, 6, 5, 20
BLOCK, TILE_W, TILE_H, TAIL_TEXELS, TAIL_INPUT = 256, 64, 4, 4096, 4096   # kernels_bloom.hip / kernels_bloom.h


# SPCBPT_BLOOM_TAIL: the most texels the fused tail's input level may hold (0: no tail).  At 1920 x 1080 the levels hold 518 400, 129 600,
# 32 400, 8 160, 2 040 and 510 texels.
VARIANTS = (("4096", "fused tail from level 5 (11 launches; the default)"), ("16384", "fused tail from level 4 (9 launches)"), ("0", "per-level kernels only (12 launches)"))


def image():
    rng = np.random.default_rng(8)
    img = np.ones((H, W, 4), np.float32)
    img[..., :3] = (2.0 ** rng.uniform(-10.0, 6.0, (H, W, 1)) * rng.uniform(0.2, 1.0, (H, W, 3))).astype(np.float32)
    img[rng.integers(0, H, 64), rng.integers(0, W, 64), :3] *= 4096.0     # small emitters far above the key
    return img


def renderer():
    import __graft_entry__ as g
    pkg = g.load_package()
    return pkg, pkg.Renderer(pkg.scenes.cornell_box(), 0)


def spans(r, names):
    return ", ".join("%s %.4f ms (%d)" % ((n,) + r.kernel_time(n)) for n in names)


def run_spans():
    pkg, r = renderer()
    img = image()
    for tail, _ in VARIANTS:
        os.environ["SPCBPT_BLOOM_TAIL"] = tail
        for _ in range(WARM):
            r.bloom_image(img, levels=LEVELS)
            r.display_image(img, auto=True)
            r.sync()
    r.enable_kernel_timing(True)
    for p in range(2):
        r.reset_kernel_time()
        for _ in range(CALLS):
            r.display_image(img, auto=True)
            r.sync()
        print(f"{W}x{H} display_image, auto, pass {p}: " + spans(r, ("display_hist", "display")), flush=True)
        for tail, label in VARIANTS:
            os.environ["SPCBPT_BLOOM_TAIL"] = tail
            r.reset_kernel_time()
            for _ in range(CALLS):
                r.bloom_image(img, levels=LEVELS)
                r.sync()
            print(f"{W}x{H} bloom_image, L = {LEVELS}, {label}, pass {p}: " + spans(r, ("bloom",)), flush=True)
    r.enable_kernel_timing(False)
    del os.environ["SPCBPT_BLOOM_TAIL"]
    r.bloom_image(img, levels=LEVELS)
    a = r.read_bloom()
    os.environ["SPCBPT_BLOOM_TAIL"] = "0"
    r.bloom_image(img, levels=LEVELS)
    b = r.read_bloom()
    print("the two forms return the same bytes:", a.tobytes() == b.tobytes(), "; equal to bloom_host:", a.tobytes() == pkg.api.bloom_host(img, levels=LEVELS).tobytes(), flush=True)


def run_profile():
    _, r = renderer()
    img = image()
    for _ in range(WARM + CALLS):
        r.display_image(img, auto=True)
        r.sync()
    for _ in range(WARM + CALLS):
        r.bloom_image(img, levels=LEVELS)
        r.sync()


def plan():
    """Expected launches of one bloom call: {(kernel, grid threads): (label, bytes)} from the level sizes, as ctx_bloom.hip queues them."""
    w, h = [W], [H]
    for k in range(1, LEVELS + 1):
        w.append((w[-1] + 1) // 2)
        h.append((h[-1] + 1) // 2)
    n = [a * b for a, b in zip(w, h)]
    j, held = 0, 0
    for k in range(LEVELS, 1, -1):
        held += n[k]
        if held > TAIL_TEXELS or n[k - 1] > TAIL_INPUT:
            break
        j = k - 1
    out = {}
    last_down = j if j else LEVELS
    for k in range(1, last_down + 1):
        tiles = -(-w[k] // TILE_W) * -(-h[k] // TILE_H)
        out[("k_bloom_down", tiles * BLOCK)] = (f"down {k - 1} -> {k} ({w[k]} x {h[k]})", 16 * (n[k - 1] + n[k]))
    if j:
        out[("k_bloom_tail", 1024)] = (f"tail from level {j} ({w[j]} x {h[j]}; levels {j + 1} .. {LEVELS} in LDS)", 16 * 3 * n[j])
    for k in range(last_down - 1, 0, -1):
        out[("k_bloom_up", -(-n[k] // BLOCK) * BLOCK)] = (f"up-and-mix level {k} ({w[k]} x {h[k]})", 16 * (2 * n[k] + n[k + 1]))
    out[("k_bloom_composite", -(-n[0] // BLOCK) * BLOCK)] = (f"composite ({W} x {H})", 16 * (2 * n[0] + n[1]))
    out[("k_display_map", -(-n[0] // BLOCK) * BLOCK)] = (f"k_display_map ({W} x {H})", 20 * n[0])
    out[("k_display_histogram", 1024 * BLOCK)] = (f"k_display_histogram ({W} x {H})", 16 * n[0])
    return out


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
    agg = {}
    for row in rows:
        name = row["Kernel_Name"]
        short = next((s for s in ("k_bloom_down", "k_bloom_up", "k_bloom_tail", "k_bloom_composite", "k_display_map", "k_display_histogram", "k_display_exposure") if s in name), None)
        if not short:
            continue
        grid = int(row.get("Grid_Size_X") or row.get("Grid_Size") or 0)
        agg.setdefault((short, grid), []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]) - int(row["Start_Timestamp"])))
    expected = plan()
    print(f"{W}x{H}, L = {LEVELS}: kernel trace of {WARM + CALLS} display_image (auto) and {WARM + CALLS} bloom_image calls; the last {CALLS} launches of each kernel")
    total = 0.0
    for key, v in sorted(agg.items(), key=lambda kv: min(t for t, _ in kv[1])):
        v.sort()
        per_call = len(v) / (WARM + CALLS)
        timed = [dt for _, dt in v[-int(round(CALLS * per_call)):]]
        mean_us = sum(timed) / len(timed) / 1e3
        label, nbytes = expected.get(key, (f"{key[0]} grid {key[1]}", 0))
        if key[0].startswith("k_bloom"):
            total += mean_us * per_call
        bw = f"{nbytes / 1e6:8.2f} MB  {nbytes / (mean_us * 1e-6) / 1e12:6.3f} TB/s" if nbytes else "       -"
        print(f"  {key[0]:20s} {label:62s} {per_call:4.1f} per call  mean {mean_us:8.2f} us  min {min(timed) / 1e3:8.2f} us  {bw}")
    print(f"  sum of the bloom kernels' mean times per call: {total:.2f} us in {sum(len(v) for k, v in agg.items() if k[0].startswith('k_bloom')) / (WARM + CALLS):.0f} launches")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "spans"
    if mode == "spans":
        run_spans()
    elif mode == "profile":
        run_profile()
    elif mode == "report":
        report(sys.argv[2])
    else:
        sys.exit(__doc__)
