"""What the information gain of candidate viewpoints costs (kicp_grid_gain), one process, the caller bound as tools/bench_pipeline.py
binds it.

Cases: tools/bench_clearance.py's - the grid left by a short drive in cfg1's scene and in cfg4's, each at 0.05 m and 0.25 m cells.  The
viewpoints are what an exploration node would ask about: the best cells of the frontiers under tools/bench_potential.py's plan with the
robot's cell as the one goal (word 9 of kicp_grid_frontiers' rows), and a lattice of clear cells over the grid, up to 1 024 together.
Two ranges: 8 m in cells, capped at the 361 the entry takes, and 20 cells - at which 20 of a wave's 64 lanes have a step to take.
Per case and range, the host clock around the call, which returns after its kernels have completed and the rows have arrived:
  - kicp_grid_gain;
  - the host route: kicp_grid_occupancy (the readout on the GPU and its copy) then kicp_gain_from_occupancy, single-threaded - the
    comparison; and that second call alone.
The results are checked equal inside the tool.  The C entries are called with arrays allocated once per case, so no call pays for fresh
pages of the allocator's.  Warm; the calls of every case alternate `rounds` times; median, p10 / p90, min .. max.  Prints one JSON line.

    python tools/bench_gain.py [--rounds 10] [--frames 8] [--views 1024]
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
from bench_potential import KW, plan  # noqa: E402
from bench_relocalize import spread  # noqa: E402

U32 = C.POINTER(C.c_uint)
RANGE_M, SMALL_RANGE, MAX_RANGE = 8.0, 20, 361


def viewpoints(c, weight, limit):
    """the frontiers' best cells under a plan from the robot's cell, then clear cells on a lattice fine enough to fill `limit`"""
    _, start, _, _ = plan(c, weight)
    c["grid"].potential(c["table"], weight, [start], **KW)  # leaves the plan in the handle
    best = c["grid"].frontiers(use_plan=True)[:, 9].astype(np.uint32)[:limit]
    occ = c["grid"].occupancy()
    clear = (occ >= 0) & (occ <= 65)
    step = max(1, int(np.sqrt(clear.sum() / max(1, limit - len(best)))))
    ys, xs = np.nonzero(clear[::step, ::step])
    lattice = (ys * step * occ.shape[1] + xs * step).astype(np.uint32)[:limit - len(best)]
    return start, len(best), np.ascontiguousarray(np.concatenate([best, lattice]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--views", type=int, default=1024)
    a = ap.parse_args()
    bind, where = placement()
    if bind:
        bind()
    lib, weight = K.lib(), K.plan_weights()
    todo = cases(a.frames)
    names = ("device", "host_route", "host_alone")
    for c in todo:
        c["start"], c["n_frontiers"], c["views"] = viewpoints(c, weight, a.views)
        shape = (c["cfg"]["height"], c["cfg"]["width"])
        c["occ"] = np.empty(shape, dtype=np.int8)
        c["ranges"] = sorted({SMALL_RANGE, min(MAX_RANGE, int(round(RANGE_M / c["cell"])))})
        c["cfgs"] = {R: K.GainConfig(1, 0.65, R) for R in c["ranges"]}
        c["rows"] = [np.zeros((len(c["views"]), K.GAIN_WORDS), dtype=np.uint32) for _ in range(2)]
        c["t"] = {(R, name): [] for R in c["ranges"] for name in names}
        c["result"] = {}
    for r in range(a.rounds + 2):  # (the first two rounds warm)
        print("round %d of %d" % (r + 1, a.rounds + 2), file=sys.stderr, flush=True)
        for c in todo:
            h, rows, views, n, cells = c["grid"]._h, c["rows"], c["views"], len(c["views"]), c["occ"].size
            for R in c["ranges"]:
                cfg = c["cfgs"][R]
                t = [time.perf_counter()]
                rc = [lib.kicp_grid_gain(h, C.byref(cfg), views.ctypes.data_as(U32), n, rows[0].ctypes.data_as(U32), rows[0].size)]
                t.append(time.perf_counter())
                rc.append(lib.kicp_grid_occupancy(h, 1, c["occ"].ctypes.data_as(C.POINTER(C.c_byte)), cells))
                middle = time.perf_counter()
                rc.append(lib.kicp_gain_from_occupancy(c["occ"].ctypes.data_as(C.POINTER(C.c_byte)), c["occ"].shape[1], c["occ"].shape[0], C.byref(cfg),
                                                       views.ctypes.data_as(U32), n, rows[1].ctypes.data_as(U32), rows[1].size))
                t.append(time.perf_counter())
                if r == 0:
                    assert rc == [0] * 3, rc
                    assert np.array_equal(rows[0], rows[1]), np.flatnonzero((rows[0] != rows[1]).any(axis=1))[:8]
                    assert np.array_equal(K.gain_from_occupancy(c["occ"], views, R), rows[1]) and np.array_equal(c["grid"].gain(views, R), rows[0])
                    walked = rows[1][:, 3] == 0
                    c["result"][R] = {"clear_viewpoints": int(walked.sum()), "seen_median": float(np.median(rows[1][walked, 0])) if walked.any() else 0.0,
                                      "seen_max": int(rows[1][:, 0].max()), "rays_blocked_share": float(rows[1][walked, 1].sum() / max(1, 8 * R * walked.sum())),
                                      "rays_left_share": float(rows[1][walked, 2].sum() / max(1, 8 * R * walked.sum()))}
                if r >= 2:
                    c["t"][(R, "device")].append((t[1] - t[0]) * 1e3)
                    c["t"][(R, "host_route")].append((t[2] - t[1]) * 1e3)
                    c["t"][(R, "host_alone")].append((t[2] - middle) * 1e3)
    out = []
    for c in todo:
        for R in c["ranges"]:
            out.append({"scene": c["name"], "points": c["points"], "frames": a.frames, "cell_m": c["cell"], "grid_cells": [c["cfg"]["width"], c["cfg"]["height"]],
                        "robot_cell": list(c["start"]), "viewpoints": len(c["views"]), "of_them_frontier_best_cells": c["n_frontiers"], "range_cells": R, **c["result"][R],
                        "grid_gain_ms": spread(c["t"][(R, "device")]), "host_occupancy_then_gain_ms": spread(c["t"][(R, "host_route")]),
                        "host_gain_from_occupancy_alone_ms": spread(c["t"][(R, "host_alone")])})
    print(json.dumps({"caller_process": where, "rounds": a.rounds, "gain": out}))


if __name__ == "__main__":
    main()
