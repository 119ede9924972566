"""What the transient obstacles cost (kicp_grid_transients_device) beside what a frame costs anyway, one process, the caller bound as
tools/bench_pipeline.py binds it.

Cases: tools/bench_clearance.py's - the grid left by a short drive in cfg1's scene and in cfg4's, each at 0.05 m and 0.25 m cells.  The
frame is the drive's next scan with a box of returns (0.5 m x 0.5 m, 400 points) added where the grid reads free, two metres from the
robot; it lies in HBM.  Per case, the host clock around the call, which returns with the grid's stream drained:
  - kicp_grid_transients_device of that frame (min_observations 1, free_max 25, min_points 3, min_size 3), rows only;
  - kicp_grid_integrate_device of the same frame, into a second grid with the same counters, so that the first one's stay as they are;
  - kicp_grid_frontiers on the same grid, rows only: the union-find's grid-wide launches are the same in both;
  - kicp_grid_costmap over the last frame's window grown by R, with the switch off and on (the plane holds the box).
The device rows are checked against kicp_transients_from_counts inside the tool.  Warm; the calls of every case alternate `rounds`
times; median, p10 / p90, min .. max.  Prints one JSON line.

    python tools/bench_transients.py [--rounds 30] [--frames 8]
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
from kinematic_icp_amd import synthetic as syn  # noqa: E402
from bench_clearance import cases  # noqa: E402
from bench_grid import make_grid, scene_and_beams  # noqa: E402
from bench_pipeline import placement  # noqa: E402
from bench_relocalize import spread  # noqa: E402

PARAMS = dict(min_observations=1, free_max=25, min_points=3, min_size=3)
U64, DP = C.POINTER(C.c_ulonglong), C.POINTER(C.c_double)


def frame_with_box(c):
    """the drive's next scan in the base frame with a box of returns where the grid reads free -> (points, pose, sensor)"""
    cfg, scene, dirs, rng = scene_and_beams(c["name"])
    pose = syn.pose_mul(c["pose"], syn.planar_pose(0.2, 0.0, np.deg2rad(2.0)))
    scan = syn.make_scan(scene, pose, dirs, cfg.sensor_height, rng)
    g, occ = c["cfg"], c["grid"].occupancy(1)
    free = (occ >= 0) & (occ <= PARAMS["free_max"])
    k = max(int(round(0.25 / g["cell"])), 1)  # half the box in cells
    ahead = syn.pose_act(pose, np.array([[2.0, 0.0, 0.0]]))[0]
    yy, xx = np.nonzero(free)
    order = np.argsort(np.hypot(g["origin_x"] + (xx + 0.5) * g["cell"] - ahead[0], g["origin_y"] + (yy + 0.5) * g["cell"] - ahead[1]))
    for i in order:
        x, y = int(xx[i]), int(yy[i])
        if k <= x < g["width"] - k and k <= y < g["height"] - k and free[y - k:y + k + 1, x - k:x + k + 1].all():
            break
    else:
        raise SystemExit("no free patch for the box in %s at %g m" % (c["name"], g["cell"]))
    centre = np.array([g["origin_x"] + (x + 0.5) * g["cell"], g["origin_y"] + (y + 0.5) * g["cell"]])
    world = np.concatenate([centre + rng.uniform(-0.25, 0.25, (400, 2)), np.full((400, 1), 0.0)], axis=1)
    box = syn.pose_act(syn.pose_inverse(pose), world)
    box[:, 2] = 0.5 * (g["z_min"] + g["z_max"])
    return np.ascontiguousarray(np.concatenate([scan, box])), pose, np.array([0.0, 0.0, cfg.sensor_height])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--frames", type=int, default=8)
    a = ap.parse_args()
    bind, where = placement()
    if bind:
        bind()
    todo = cases(a.frames)
    names = ("transients", "integrate", "frontiers", "costmap_off", "costmap_on")
    kw = dict(min_observations=1, occupied_thresh=0.65, unknown_is_obstacle=False, inflate_unknown=True)
    for c in todo:
        g = c["cfg"]
        points, c["frame_pose"], c["sensor"] = frame_with_box(c)
        c["frame"], c["frame_points"] = K.DeviceFrame(points), len(points)
        c["counts"] = c["grid"].counts()
        c["other"] = make_grid(g)  # takes the frame again and again; its counters saturate no sooner than after 65 535 rounds
        c["other"].set_counts(c["counts"])
        args = (g["cell"], g["origin_x"], g["origin_y"], g["width"], g["height"], g["z_min"], g["z_max"], g["max_ray"])
        host = K.transients_from_counts(c["counts"], args, points, c["frame_pose"], c["sensor"], return_stats=True, return_plane=True, **PARAMS)
        rows, stats = c["grid"].transients_device(c["frame"], c["frame_pose"], c["sensor"], return_stats=True, **PARAMS)
        assert np.array_equal(rows, host[0]) and stats == host[1] and np.array_equal(c["grid"].transient_plane(), host[2])
        assert len(rows) >= 1 and rows[:, 2].max() >= 200, rows  # the box is among them
        # the two entries with rows are called with arrays allocated once and large enough, so no call runs twice
        c["cap"] = max(len(rows), len(c["grid"].frontiers())) + 1
        c["rows"] = np.zeros((c["cap"], 10), dtype=np.uint64)
        c["pose_c"], c["sensor_c"] = np.ascontiguousarray(c["frame_pose"], dtype=np.float64), np.ascontiguousarray(c["sensor"], dtype=np.float64)
        c["result"] = {"points_used": stats[0], "points_inside": stats[1], "cells_with_a_return": stats[2], "transient_cells": stats[3], "transients": int(len(rows)),
                       "largest_transient_cells": int(rows[:, 1].max()), "most_returns": int(rows[:, 2].max()), "plane_cells": int(host[2].sum())}
        c["t"] = {name: [] for name in names}
    lib, tcfg, fcfg = K.lib(), K.TransientConfig(**PARAMS), K.FrontierConfig(1, 0.65, 1)
    for r in range(a.rounds + 3):  # (the first three rounds warm)
        for c in todo:
            grid, rect, n = c["grid"], c["rects"]["window"], [C.c_size_t(), C.c_size_t()]
            t = [time.perf_counter()]
            rc = [lib.kicp_grid_transients_device(grid._h, c["frame"].ptr, c["frame"].n, c["pose_c"].ctypes.data_as(DP), c["sensor_c"].ctypes.data_as(DP), C.byref(tcfg),
                                                  c["rows"].ctypes.data_as(U64), c["cap"], C.byref(n[0]), None, 0, None)]
            t.append(time.perf_counter())
            c["other"].integrate_device(c["frame"], c["frame_pose"], c["sensor"])
            t.append(time.perf_counter())
            rc.append(lib.kicp_grid_frontiers(grid._h, C.byref(fcfg), 0, c["rows"].ctypes.data_as(U64), c["cap"], C.byref(n[1]), None, 0))
            t.append(time.perf_counter())
            assert rc == [0, 0] and n[0].value == c["result"]["transients"], (rc, n[0].value)
            off = grid.costmap(c["table"], rect=rect, **kw)
            t.append(time.perf_counter())
            grid.use_transients(True)
            t.append(time.perf_counter())
            on = grid.costmap(c["table"], rect=rect, **kw)
            t.append(time.perf_counter())
            grid.use_transients(False)
            if r == 0:
                c["result"]["costmap_cells_changed_by_the_switch"] = int((on != off).sum())
                assert c["result"]["costmap_cells_changed_by_the_switch"] > 0 and np.array_equal(grid.counts(), c["counts"])
            if r >= 3:
                for k, name in enumerate(names[:4]):
                    c["t"][name].append((t[k + 1] - t[k]) * 1e3)
                c["t"]["costmap_on"].append((t[6] - t[5]) * 1e3)
    out = []
    for c in todo:
        out.append({"scene": c["name"], "points": c["frame_points"], "frames": a.frames, "cell_m": c["cell"], "grid_cells": [c["cfg"]["width"], c["cfg"]["height"]],
                    "radius_cells": c["radius"], "cells_window_grown": int(c["rects"]["window"][2] * c["rects"]["window"][3]), **c["result"],
                    "grid_transients_device_ms": spread(c["t"]["transients"]), "grid_integrate_device_ms": spread(c["t"]["integrate"]),
                    "grid_frontiers_ms": spread(c["t"]["frontiers"]), "costmap_window_switch_off_ms": spread(c["t"]["costmap_off"]),
                    "costmap_window_switch_on_ms": spread(c["t"]["costmap_on"])})
    print(json.dumps({"caller_process": where, "rounds": a.rounds, "transients": out}))


if __name__ == "__main__":
    main()
