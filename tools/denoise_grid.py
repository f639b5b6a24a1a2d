"""The grid behind the denoiser's default parameters (include/spcbpt.h): RMSE of the denoised 4-frame "pt" image of the
Cornell box at 64 x 64 against a disjoint 512-frame mean, for sigma_c in {1, 2, 4} x sigma_n in {0.25, 0.5, 1} x sigma_x in
{0.01, 0.03, 0.1} of the bounding-box diagonal, and the denoised / noisy ratios of the defaults on the Cornell box and the textured
bedroom.  Then the grid behind SPCBPT_DENOISE_SIGMA_V: the variance-guided filter (spcbpt_denoise_variance) for sigma_v in
{2, 4, 8} on the same box at 4 and at 64 frames against a 512-frame mean disjoint from both; the default is the value with the lowest
sum of the two RMSEs.  Needs a GPU.   python tools/denoise_grid.py"""
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


def variance_grid(scene, w=64, h=64, counts=(4, 64), sigmas=(2.0, 4.0, 8.0)):
    r = setup(scene, w, h)
    r.set_film_moments(True)
    shots = {}
    for f in range(max(counts)):
        r.launch("pt", f)
        r.launch_features(f)
        if f + 1 in counts:
            s = {"film": r.read_accum()[..., :3].astype(np.float64), "error": r.film_error()["mean"]}
            for sv in sigmas:
                r.denoise_variance(5, sv)
                s[sv] = r.read_denoised()[0][..., :3].astype(np.float64)
            r.denoise(5)
            s["plain"] = r.read_denoised()[0][..., :3].astype(np.float64)
            shots[f + 1] = s
    n0 = max(counts)
    for f in range(n0, n0 + REF):
        r.launch("pt", f)
    ref = ((n0 + REF) * r.read_accum()[..., :3].astype(np.float64) - n0 * shots[n0]["film"]) / REF
    print(f"variance-guided filter, cornell {w}x{h}, RMSE against a disjoint {REF}-frame mean:")
    for n in counts:
        s = shots[n]
        print(f"  {n} frames (film error {s['error']:.4f}): film {rmse(s['film'], ref):.5f}, plain a-trous {rmse(s['plain'], ref):.5f}, "
              + ", ".join(f"sigma_v {sv:g}: {rmse(s[sv], ref):.5f}" for sv in sigmas))
    for sv in sorted(sigmas, key=lambda sv: sum(rmse(shots[n][sv], ref) for n in counts)):
        print(f"  sigma_v {sv:g}: sum over {counts} frames {sum(rmse(shots[n][sv], ref) for n in counts):.5f}")


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
    variance_grid(scene)


if __name__ == "__main__":
    main()
