"""What the grid's costmap costs (kicp_grid_costmap), one process, the caller bound as tools/bench_pipeline.py binds it.

Cases: the grid left by a short drive in cfg1's scene (64 beams x 2048 azimuths) and in cfg4's (a 1 080-beam scan), each at 0.05 m and
0.25 m cells (tools/bench_grid.py's scenes, bands and grids; max_ray is 12 m here, so that a frame's window is a part of the grid and
not all of it).  R is the number of cells in 1 m; the table is Nav2's (inscribed radius 0.35 m, cost
scaling factor 3).  Per case, the host clock around the call, which returns after its kernels have completed and the bytes have arrived:
  - kicp_grid_costmap over the full grid, and over the last frame's window grown by R and clipped (what a node refreshes per frame);
  - the same two rectangles by kicp_grid_occupancy + kicp_grid_costmap_from_occupancy: the readout over PCIe, then the transform on the
    host, single-threaded (what a node had to do before) - its result is checked against the device's.
Warm; the four calls of every case alternate `rounds` times; median, p10 / p90, min .. max.  Prints one JSON line.

    python tools/bench_clearance.py [--rounds 30] [--frames 8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kinematic_icp_amd as K  # noqa: E402
from kinematic_icp_amd import synthetic as syn  # noqa: E402
from bench_grid import CELLS, GEOMETRY, make_grid, scene_and_beams  # noqa: E402
from bench_pipeline import placement  # noqa: E402
from bench_relocalize import spread  # noqa: E402
import grid_ref as gr  # noqa: E402

MAX_RAY = 12.0


def grid_config(name, cell):
    _, _, (z_min, z_max), _, half = GEOMETRY[name]
    side = int(round(2.0 * half / cell))
    return gr.make_config(cell, -half, -half, side, side, z_min, z_max, MAX_RAY)


def grown(rect, radius, width, height):
    x0, y0, w, h = rect
    ax, ay = max(x0 - radius, 0), max(y0 - radius, 0)
    return (ax, ay, min(x0 + w + radius, width) - ax, min(y0 + h + radius, height) - ay)


def cases(n_frames, only=None):
    """only: (scene, cell) pairs to build instead of all four"""
    out = []
    for name in GEOMETRY:
        if only is not None and not any(scene == name for scene, _ in only):
            continue
        cfg, scene, dirs, rng = scene_and_beams(name)
        sensor = np.array([0.0, 0.0, cfg.sensor_height])
        poses = [syn.planar_pose(1.2, -0.7, 0.9)]
        for k in range(1, n_frames):
            poses.append(syn.pose_mul(poses[-1], syn.planar_pose(0.2, 0.0, np.deg2rad(1.0 + 0.1 * k))))
        frames = [np.ascontiguousarray(syn.make_scan(scene, pose, dirs, cfg.sensor_height, rng)) for pose in poses]
        for cell in CELLS:
            if only is not None and (name, cell) not in only:
                continue
            gcfg = grid_config(name, cell)
            grid = make_grid(gcfg)
            for pose, frame in zip(poses, frames):
                grid.integrate(frame, pose, sensor)
            radius = int(round(1.0 / cell))
            window = grid.last_window()
            out.append(dict(name=name, cell=cell, cfg=gcfg, grid=grid, radius=radius, table=K.nav2_cost_table(cell, radius, 0.35, 3.0), points=len(frames[0]),
                            rects={"full": None, "window": grown(window, radius, gcfg["width"], gcfg["height"])}, window=window, pose=poses[-1],
                            t={(where, which): [] for where in ("device", "host") for which in ("full", "window")}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--frames", type=int, default=8)
    a = ap.parse_args()
    bind, where = placement()
    if bind:
        bind()
    todo = cases(a.frames)
    kw = dict(min_observations=1, occupied_thresh=0.65, unknown_is_obstacle=False, inflate_unknown=True)
    for r in range(a.rounds + 3):  # (the first three rounds warm)
        for c in todo:
            for which, rect in c["rects"].items():
                t0 = time.perf_counter()
                dev = c["grid"].costmap(c["table"], rect=rect, **kw)
                t1 = time.perf_counter()
                host = K.costmap_from_occupancy(c["grid"].occupancy(1), c["table"], rect=rect, **kw)
                t2 = time.perf_counter()
                if r == 0:
                    assert np.array_equal(dev, host)
                    c["cells_" + which] = int(dev.size)
                    if rect is None:
                        c["classes"] = {"lethal": int((dev == 254).sum()), "inflated": int(((dev > 0) & (dev < 254)).sum()), "no_information": int((dev == 255).sum()),
                                        "free": int((dev == 0).sum())}
                if r >= 3:
                    c["t"]["device", which].append((t1 - t0) * 1e3), c["t"]["host", which].append((t2 - t1) * 1e3)
    rows = []
    for c in todo:
        rows.append({"scene": c["name"], "points": c["points"], "frames": a.frames, "cell_m": c["cell"], "grid_cells": [c["cfg"]["width"], c["cfg"]["height"]],
                     "max_ray_m": MAX_RAY, "radius_cells": c["radius"], "last_window": list(c["window"]), "cells_full": c["cells_full"], "cells_window_grown": c["cells_window"],
                     "costs_full": c["classes"],
                     "costmap_full_ms": spread(c["t"]["device", "full"]), "costmap_window_ms": spread(c["t"]["device", "window"]),
                     "host_readout_and_costmap_full_ms": spread(c["t"]["host", "full"]), "host_readout_and_costmap_window_ms": spread(c["t"]["host", "window"])})
    print(json.dumps({"caller_process": where, "rounds": a.rounds, "costmap": rows}))


if __name__ == "__main__":
    main()
