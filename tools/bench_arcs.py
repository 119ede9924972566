"""What scoring a fan of arc trajectories on the grid's plan costs (kicp_grid_score_arcs), one process, the caller bound as
tools/bench_pipeline.py binds it.

Case: tools/bench_potential.py's first - the grid left by a short drive in cfg1's scene at 0.05 m cells, R the number of cells in 1 m,
Nav2's cost table, inflate_unknown on, NavFn's weights, the goal the cell of the explored area farthest from the robot - whose
kicp_grid_potential leaves the plan in the handle.  The fan: K commands, v from 0 to 1.5 m/s and omega across +-1.5 rad/s on a
lattice (16 x 16, 64 x 64, 128 x 256), T = 32 steps of dt = 0.1 s from the pose the robot stands at, under a 1.0 x 0.6 m box sampled at
0.05 m (21 x 13 samples).  Per K, the host clock around the call:
  - kicp_grid_score_arcs: on the plan where it lies in HBM; returns after the K x 4 words have arrived;
  - kicp_score_arcs_from_plan: the same arithmetic on the host, one thread, over the same arrays (q = kicp_plan_q of the costmap, the
    potential as kicp_grid_potential returned it) - the comparison; its values are checked against the device's;
  - what the host route needs first, the plan's 5 bytes per cell from HBM to the caller's memory.  No entry copies q itself, so two
    entries that move as many bytes stand in: kicp_grid_counts (4 bytes per cell, a potential's size) and kicp_grid_occupancy (1 byte
    per cell, with its readout kernel in front).
The same fans once more on an OPEN FLOOR - a second handle of the same geometry whose plan is kicp_grid_potential_of_costmap over a
costmap of zeros, so that no arc collides before it leaves the grid and every pose of every arc is looked up: the most a call of
this shape can cost.  There the host entry takes seconds, so it is timed in 5 of the rounds only.
Every entry writes into an array allocated once (`out=`).  Warm; the calls alternate `rounds` times; median, p10 / p90, min .. max.
Prints one JSON line.

    python tools/bench_arcs.py [--rounds 30] [--frames 8]
"""
import argparse
import ctypes as C
import json
import math
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
from bench_grid import make_grid  # noqa: E402
from bench_pipeline import placement  # noqa: E402
from bench_potential import KW, plan  # noqa: E402
from bench_relocalize import spread  # noqa: E402

FANS = ((16, 16), (64, 64), (128, 256))  # v x omega
N_STEPS, DT = 32, 0.1
BOX = (-0.5, 0.5, -0.3, 0.3, 0.05)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--frames", type=int, default=8)
    a = ap.parse_args()
    bind, where = placement()
    if bind:
        bind()
    weight = K.plan_weights()
    c = cases(a.frames, only=[("cfg1", 0.05)])[0]
    grid, cfg = c["grid"], c["cfg"]
    costmap, _, goal, _ = plan(c, weight)
    potential = grid.potential(c["table"], weight, [goal], **KW)  # leaves the plan
    q = K.plan_q(costmap, weight)
    pose = c["pose"]
    start = K.arc_start(pose[4], pose[5], 2.0 * math.atan2(pose[2], pose[3]))
    footprint = K.footprint_box(*BOX)
    geometry = (cfg["cell"], cfg["origin_x"], cfg["origin_y"])
    counts, occupancy = np.empty(costmap.shape + (2,), dtype=np.uint16), np.empty(costmap.shape, dtype=np.int8)
    open_grid, open_costmap = make_grid(cfg), np.zeros_like(costmap)
    open_potential = open_grid.potential_of_costmap(open_costmap, weight, [goal])
    open_q = K.plan_q(open_costmap, weight)
    fans = []
    for floor, (g, fq, fpot) in (("drive", (grid, q, potential)), ("open", (open_grid, open_q, open_potential))):
        for nv, nw in FANS:
            v, omega = np.meshgrid(np.linspace(0.0, 1.5, nv), np.linspace(-1.5, 1.5, nw), indexing="ij")
            arcs = K.arc_steps(v.ravel(), omega.ravel(), DT)
            fans.append(dict(floor=floor, grid=g, q=fq, potential=fpot, arcs=arcs, dev=np.empty((len(arcs), 4), dtype=np.uint32), host=np.empty((len(arcs), 4), dtype=np.uint32),
                             t={"device": [], "host": [], "copies": []}))
    for r in range(a.rounds + 3):  # (the first three rounds warm)
        for f in fans:
            host_too = f["floor"] == "drive" or r < 8
            t = [time.perf_counter()]
            f["grid"].score_arcs(start, f["arcs"], N_STEPS, footprint, out=f["dev"])
            t.append(time.perf_counter())
            if host_too:
                K.score_arcs_from_plan(f["q"], f["potential"], *geometry, start, f["arcs"], N_STEPS, footprint, out=f["host"])
            t.append(time.perf_counter())
            K.lib().kicp_grid_counts(grid._h, counts.ctypes.data_as(C.POINTER(C.c_ushort)), costmap.size)
            K.lib().kicp_grid_occupancy(grid._h, 1, occupancy.ctypes.data_as(C.POINTER(C.c_byte)), costmap.size)
            t.append(time.perf_counter())
            if r == 0:
                assert np.array_equal(f["dev"], f["host"])
                free = f["dev"][:, 0]
                best = K.arcs_best(f["dev"], N_STEPS, w_potential=1, w_cost=1, w_blocked=1000)
                f["result"] = {"arcs_that_end_early_share": float((free < N_STEPS).mean()), "arcs_that_collide_at_step_1_share": float((free == 0).mean()),
                               "mean_free_steps": float(free.mean()), "footprint_lookups_at_most": int(np.minimum(free.astype(np.int64) + 1, N_STEPS).sum()) * len(footprint),
                               "best_arc": best, "best_arc_result": None if best is None else f["dev"][best].tolist()}
            if r >= 3:
                for k, name in enumerate(("device", "host", "copies")):
                    if name != "host" or host_too:
                        f["t"][name].append((t[k + 1] - t[k]) * 1e3)
    rows = [{"floor": f["floor"], "host_rounds": len(f["t"]["host"]), "arcs": len(f["arcs"]), "steps": N_STEPS, "dt_s": DT, "footprint_samples": len(footprint), **f["result"], "grid_score_arcs_ms": spread(f["t"]["device"]),
             "host_score_arcs_from_plan_ms": spread(f["t"]["host"]), "copies_of_5_bytes_per_cell_ms": spread(f["t"]["copies"]),
             "host_over_device": float(np.median(f["t"]["host"])) / float(np.median(f["t"]["device"]))} for f in fans]
    print(json.dumps({"caller_process": where, "rounds": a.rounds, "scene": c["name"], "frames": a.frames, "cell_m": c["cell"], "grid_cells": [cfg["width"], cfg["height"]],
                      "goal": list(goal), "start": [float(v) for v in start], "passable_cells": int((q > 0).sum()), "arcs": rows}))


if __name__ == "__main__":
    main()
