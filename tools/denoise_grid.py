"""The grid behind the denoiser's default parameters (include/spcbpt.h): RMSE of the denoised 4-frame "pt" image of the
Cornell box at 64 x 64 against a disjoint 512-frame mean, for sigma_c in {1, 2, 4} x sigma_n in {0.25, 0.5, 1} x sigma_x in
{0.01, 0.03, 0.1} of the bounding-box diagonal, and the denoised / noisy ratios of the defaults on the Cornell box and the textured
bedroom.  Needs a GPU.   python tools/denoise_grid.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g   # noqa: E402

pkg = g.load_package()
FRAMES, REF = 4, 512


def setup(scene, w, h):
    cam = scene.camera
    r = pkg.Renderer(scene, 0)
    U, V, W = pkg.camera_frame(cam["eye"], cam["lookat"], cam["up"], cam["fov"], w / h)
    r.set_camera(np.array(cam["eye"], np.float32), U, V, W)
    r.resize(w, h)
    return r


def run(scene, w=64, h=64):
    r = setup(scene, w, h)
    for f in range(FRAMES):
        r.launch("pt", f)
        r.launch_features(f)
    a4 = r.read_accum()[..., :3].astype(np.float64)
    return r, a4


def reference(r, a4):
    n = FRAMES + REF
    for f in range(FRAMES, n):
        r.launch("pt", f)
    return (n * r.read_accum()[..., :3].astype(np.float64) - FRAMES * a4) / REF


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def main():
    scene = pkg.scenes.cornell_box()
    v = np.asarray(scene.vertices, np.float64)
    diag = float(np.linalg.norm(v.max(0) - v.min(0)))
    r, a4 = run(scene)
    grid = {}
    for sc in (1.0, 2.0, 4.0):
        for sn in (0.25, 0.5, 1.0):
            for fx in (0.01, 0.03, 0.1):
                r.denoise(5, sc, sn, fx * diag)
                grid[(sc, sn, fx)] = r.read_denoised()[0][..., :3].astype(np.float64)
    r.denoise(5)
    dflt = r.read_denoised()[0][..., :3].astype(np.float64)
    ref = reference(r, a4)
    noisy = rmse(a4, ref)
    print(f"cornell 64x64, bounding-box diagonal {diag:.4f}: RMSE of the 4-frame film {noisy:.5f}")
    for k in sorted(grid, key=lambda k: rmse(grid[k], ref)):
        print(f"  sigma_c {k[0]:g} sigma_n {k[1]:g} sigma_x {k[2]:g} x diagonal: RMSE {rmse(grid[k], ref):.5f} (ratio {rmse(grid[k], ref) / noisy:.3f})")
    print(f"defaults: RMSE {rmse(dflt, ref):.5f} (ratio {rmse(dflt, ref) / noisy:.3f})")
    room = pkg.scenes.bedroom(target_tris=20_000, tex_size=64)
    r, a4 = run(room)
    r.denoise(5)
    den = r.read_denoised()[0][..., :3].astype(np.float64)
    ref = reference(r, a4)
    print(f"bedroom 64x64: RMSE {rmse(a4, ref):.5f} -> {rmse(den, ref):.5f} (ratio {rmse(den, ref) / rmse(a4, ref):.3f})")


if __name__ == "__main__":
    main()
