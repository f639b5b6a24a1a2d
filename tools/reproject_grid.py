"""The grid behind the defaults of the history reprojection (include/spcbpt.h): sigma_n in {0.1, 0.25, 0.5} x sigma_x in
{0.002, 0.005, 0.02} of the bounding-box diagonal x max_history in {16, 32, 64}, on the Cornell box and the 20 k-triangle bedroom at
64 x 64 with 64 frames of "pt" before the move, one orbit of 2 degrees and one of 8 about the look-at point (the Cornell box about
the vertical axis, the bedroom in elevation: its eye sits in a corner).  Measured: the RMSE of resolve(1) and of resolve(8)
against a disjoint 512-frame "pt" mean at the new camera.  Every one of the eight columns ranks the 27 triples; the default is the
triple with the lowest summed rank.  Needs a GPU.   python tools/reproject_grid.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g   # noqa: E402

pkg = g.load_package()
BEFORE, REF, SHOTS = 64, 512, (1, 8)
GRID = [(sn, fx, mh) for sn in (0.1, 0.25, 0.5) for fx in (0.002, 0.005, 0.02) for mh in (16.0, 32.0, 64.0)]


def rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def orbit(eye, lookat, degrees, vertical=False):
    """The eye turned about the look-at point: about the vertical axis through it, or -- vertical -- raised in elevation at its azimuth."""
    lookat = np.asarray(lookat, np.float64)
    d = np.asarray(eye, np.float64) - lookat
    a = np.radians(degrees)
    if not vertical:
        return lookat + np.array([d[0] * np.cos(a) + d[2] * np.sin(a), d[1], -d[0] * np.sin(a) + d[2] * np.cos(a)])
    flat = np.hypot(d[0], d[2])
    e = np.arctan2(d[1], flat) + a
    dist = np.linalg.norm(d)
    return lookat + np.array([d[0] / flat * dist * np.cos(e), dist * np.sin(e), d[2] / flat * dist * np.cos(e)])


def set_camera(r, cam, eye, w, h):
    U, V, W = pkg.camera_frame(eye, cam["lookat"], cam["up"], cam["fov"], w / h)
    r.set_camera(np.array(eye, np.float32), U, V, W)


def column(scene, degrees, vertical, w=64, h=64):
    """{shot: (film RMSE, {triple: RMSE}, defaults' RMSE)} for one scene and one move."""
    cam = scene.camera
    v = np.asarray(scene.vertices, np.float64).reshape(-1, 3)
    diag = float(np.linalg.norm(v.max(0) - v.min(0)))
    r = pkg.Renderer(scene, 0)
    set_camera(r, cam, cam["eye"], w, h)
    r.resize(w, h)
    for f in range(BEFORE):
        r.launch("pt", f)
        if f == 0:
            r.launch_features(0)
    r.history_capture(BEFORE)
    set_camera(r, cam, orbit(cam["eye"], cam["lookat"], degrees, vertical), w, h)
    shots = {}
    n = max(SHOTS) + REF
    for f in range(n):
        r.launch("pt", f)
        if f == 0:
            r.launch_features(0)
        if f + 1 in SHOTS:
            s = {"film": r.read_accum()[..., :3].astype(np.float64)}
            for k in GRID + [None]:
                if k is None:
                    r.history_reproject()
                else:
                    r.history_reproject(k[0], k[1] * diag, k[2])
                r.history_resolve(f + 1)
                s[k] = r.read_history(True, False)["resolved"][..., :3].astype(np.float64)
            shots[f + 1] = s
    last = max(SHOTS)
    ref = (n * r.read_accum()[..., :3].astype(np.float64) - last * shots[last]["film"]) / REF
    r.close()
    if not all(rmse(s["film"], ref) > 0 for s in shots.values()):
        raise SystemExit(f"the camera orbited by {degrees:g} degrees sees nothing: it has left the scene")
    return {k: (rmse(s["film"], ref), {t: rmse(s[t], ref) for t in GRID}, rmse(s[None], ref)) for k, s in shots.items()}


def main():
    # the bedroom's eye sits 0.4 from two walls: 8 degrees about the vertical axis leave the room either way, so its orbits go up
    scenes = (("cornell", pkg.scenes.cornell_box(), False), ("bedroom", pkg.scenes.bedroom(target_tris=20_000, tex_size=64), True))
    columns = {}
    for name, scene, vertical in scenes:
        for degrees in (2.0, 8.0):
            for shot, c in column(scene, degrees, vertical).items():
                columns[(name, degrees, shot)] = c
    ranks = {t: 0 for t in GRID}
    for key, (film, grid, dflt) in columns.items():
        for t in GRID:   # the rank of a triple in a column: how many triples are strictly better there (ties share a rank)
            ranks[t] += sum(grid[u] < grid[t] for u in GRID)
    keys = list(columns)
    print("columns: " + ", ".join(f"{n} {d:g} deg resolve({s})" for n, d, s in keys))
    print("film:     " + " ".join(f"{columns[k][0]:.5f}" for k in keys))
    print("defaults: " + " ".join(f"{columns[k][2]:.5f}" for k in keys))
    for t in sorted(GRID, key=lambda t: ranks[t]):
        print(f"sigma_n {t[0]:g} sigma_x {t[1]:g} x diagonal max_history {t[2]:g}: rank sum {ranks[t]:3d}  " + " ".join(f"{columns[k][1][t]:.5f}" for k in keys))


if __name__ == "__main__":
    main()
