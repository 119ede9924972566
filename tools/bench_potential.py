"""What the cost-to-go field over the grid's costmap costs (kicp_grid_potential), one process, the caller bound as tools/bench_pipeline.py
binds it.

Cases: tools/bench_clearance.py's - the grid left by a short drive in cfg1's scene and in cfg4's, each at 0.05 m and 0.25 m cells, R the
number of cells in 1 m, Nav2's cost table, inflate_unknown on - with NavFn's weights (neutral 50, factor 4 / 5, lethal from 253, unknown
space impassable).  The start is the cell the robot stands in after the drive; the one goal is the cell of the explored area farthest
from it: of the cells the field reaches from the robot's cell, the one at the largest distance.  Per case, the host clock around the
call, which returns after its kernels have completed and the potentials have arrived:
  - kicp_grid_potential: costmap and field on the GPU, the costmap never leaves HBM;
  - kicp_grid_potential_of_costmap: the field on the GPU over a costmap uploaded from host memory;
  - kicp_potential_from_costmap: the field on the host over the same costmap, single-threaded (a binary-heap Dijkstra) - the comparison;
    its values are checked against the device's;
  - kicp_grid_potential with max_potential at the median of the reached cells' potentials, so that the field stops at about half the
    area;
  - kicp_grid_counts, which copies exactly as many bytes from HBM to the caller's memory as a potential has: what the copy of the
    result costs alone.
Every entry writes into an array allocated once per case (`out=`), so no call pays for fresh pages of the allocator's.
Warm; the calls of every case alternate `rounds` times; median, p10 / p90, min .. max.  Prints one JSON line.

    python tools/bench_potential.py [--rounds 30] [--frames 8]
"""
import argparse
import ctypes as C
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
from bench_clearance import cases  # noqa: E402
from bench_pipeline import placement  # noqa: E402
from bench_relocalize import spread  # noqa: E402

KW = dict(min_observations=1, occupied_thresh=0.65, unknown_is_obstacle=False, inflate_unknown=True)


def plan(c, weight):
    """the robot's cell (the middle of the last window), the goal, the clamp for half the area, and the costmap the host entries take"""
    x0, y0, w, h = c["window"]  # (these drives stay near the middle of their grids: no window is clipped)
    costmap = c["grid"].costmap(c["table"], **KW)
    start = (x0 + w // 2, y0 + h // 2)
    if weight[costmap[start[1], start[0]]] == 0:  # inflated or unseen: the nearest passable cell instead
        ys, xs = np.nonzero(weight[costmap] > 0)
        k = np.argmin((xs - start[0]) ** 2 + (ys - start[1]) ** 2)
        start = (int(xs[k]), int(ys[k]))
    from_robot = K.potential_from_costmap(costmap, weight, [start])
    ys, xs = np.nonzero(from_robot != K.UNREACHED)
    k = np.argmax((xs - start[0]) ** 2 + (ys - start[1]) ** 2)
    goal = (int(xs[k]), int(ys[k]))
    field = K.potential_from_costmap(costmap, weight, [goal])
    return costmap, start, goal, int(np.median(field[field != K.UNREACHED]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--frames", type=int, default=8)
    a = ap.parse_args()
    bind, where = placement()
    if bind:
        bind()
    weight = K.plan_weights()
    todo = cases(a.frames)
    names = ("potential", "of_costmap", "host", "clamped", "copy")
    for c in todo:
        c["costmap"], c["start"], c["goal"], c["half"] = plan(c, weight)
        c["t"] = {name: [] for name in names}
        c["out"] = [np.empty(c["costmap"].shape, dtype=np.uint32) for _ in range(4)]
        c["counts"] = np.empty(c["costmap"].shape + (2,), dtype=np.uint16)
    for r in range(a.rounds + 3):  # (the first three rounds warm)
        for c in todo:
            grid, goals, out = c["grid"], [c["goal"]], c["out"]
            t = [time.perf_counter()]
            dev, stats = grid.potential(c["table"], weight, goals, return_stats=True, out=out[0], **KW)
            t.append(time.perf_counter())
            via, via_stats = grid.potential_of_costmap(c["costmap"], weight, goals, return_stats=True, out=out[1])
            t.append(time.perf_counter())
            host, host_stats = K.potential_from_costmap(c["costmap"], weight, goals, return_stats=True, out=out[2])
            t.append(time.perf_counter())
            clamped, clamped_stats = grid.potential(c["table"], weight, goals, max_potential=c["half"], return_stats=True, out=out[3], **KW)
            t.append(time.perf_counter())
            K.lib().kicp_grid_counts(grid._h, c["counts"].ctypes.data_as(C.POINTER(C.c_ushort)), c["costmap"].size)
            t.append(time.perf_counter())
            if r == 0:
                assert np.array_equal(dev, host) and np.array_equal(via, host) and stats[:3] == via_stats[:3] == host_stats[:3]
                assert np.array_equal(clamped, K.potential_from_costmap(c["costmap"], weight, goals, c["half"]))
                path = K.potential_path(dev, c["costmap"], weight, c["start"])
                c["result"] = {"reached_cells": stats[1], "passable_cells": int((weight[c["costmap"]] > 0).sum()), "rounds": stats[3], "rounds_of_costmap": via_stats[3],
                               "potential_at_start": int(dev[c["start"][1], c["start"][0]]), "path_cells": int(len(path)),
                               "clamped": {"max_potential": c["half"], "below": clamped_stats[1], "at": clamped_stats[2], "rounds": clamped_stats[3]}}
            if r >= 3:
                for k, name in enumerate(names):
                    c["t"][name].append((t[k + 1] - t[k]) * 1e3)
    rows = []
    for c in todo:
        copy = float(np.median(c["t"]["copy"]))
        rows.append({"scene": c["name"], "points": c["points"], "frames": a.frames, "cell_m": c["cell"], "grid_cells": [c["cfg"]["width"], c["cfg"]["height"]],
                     "radius_cells": c["radius"], "start": list(c["start"]), "goal": list(c["goal"]), **c["result"],
                     "grid_potential_ms": spread(c["t"]["potential"]), "grid_potential_of_costmap_ms": spread(c["t"]["of_costmap"]),
                     "host_potential_from_costmap_ms": spread(c["t"]["host"]), "grid_potential_clamped_ms": spread(c["t"]["clamped"]),
                     "copy_of_as_many_bytes_ms": spread(c["t"]["copy"]), "copy_share_of_grid_potential": copy / float(np.median(c["t"]["potential"]))})
    print(json.dumps({"caller_process": where, "rounds": a.rounds, "potential": rows}))


if __name__ == "__main__":
    main()
