"""What the exploration frontiers of the grid cost (kicp_grid_frontiers), one process, the caller bound as tools/bench_pipeline.py binds it.

Cases: tools/bench_clearance.py's - the grid left by a short drive in cfg1's scene and in cfg4's, each at 0.05 m and 0.25 m cells.  The
plan is tools/bench_potential.py's with the robot's cell as the one goal: R the number of cells in 1 m, Nav2's cost table,
inflate_unknown on, NavFn's weights.  Per case, the host clock around the call, which returns after its kernels have completed and the
rows - and the label plane, where one is asked for - have arrived:
  - kicp_grid_frontiers without the plan and without the label plane;
  - kicp_grid_frontiers with use_plan;
  - kicp_grid_frontiers with use_plan and the label plane (width * height words more to copy);
  - the host route: kicp_grid_occupancy (the readout on the GPU and its copy) then kicp_frontiers_from_occupancy with the potential,
    single-threaded - the comparison; and that second call alone.
The results are checked equal inside the tool.  The C entries are called with arrays allocated once per case, so no call pays for fresh
pages of the allocator's.  Warm; the calls of every case alternate `rounds` times; median, p10 / p90, min .. max.  Prints one JSON line.

    python tools/bench_frontiers.py [--rounds 30] [--frames 8]
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

U64, U32 = C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--frames", type=int, default=8)
    a = ap.parse_args()
    bind, where = placement()
    if bind:
        bind()
    lib, weight = K.lib(), K.plan_weights()
    cfg = K.FrontierConfig(1, 0.65, 1)
    todo = cases(a.frames)
    names = ("plain", "use_plan", "use_plan_labels", "host_route", "host_alone")
    for c in todo:
        _, c["start"], _, _ = plan(c, weight)
        shape = (c["cfg"]["height"], c["cfg"]["width"])
        c["potential"] = c["grid"].potential(c["table"], weight, [c["start"]], **KW)  # leaves the plan in the handle
        c["cap"] = len(c["grid"].frontiers()) + 1
        c["rows"] = [np.zeros((c["cap"], K.FRONTIER_WORDS), dtype=np.uint64) for _ in range(4)]
        c["labels"], c["occ"] = np.empty(shape, dtype=np.uint32), np.empty(shape, dtype=np.int8)
        c["t"] = {name: [] for name in names}
    for r in range(a.rounds + 3):  # (the first three rounds warm)
        for c in todo:
            h, rows, cap, cells, n = c["grid"]._h, c["rows"], c["cap"], c["labels"].size, [C.c_size_t() for _ in range(4)]
            t = [time.perf_counter()]
            rc = [lib.kicp_grid_frontiers(h, C.byref(cfg), 0, rows[0].ctypes.data_as(U64), cap, C.byref(n[0]), None, 0)]
            t.append(time.perf_counter())
            rc.append(lib.kicp_grid_frontiers(h, C.byref(cfg), 1, rows[1].ctypes.data_as(U64), cap, C.byref(n[1]), None, 0))
            t.append(time.perf_counter())
            rc.append(lib.kicp_grid_frontiers(h, C.byref(cfg), 1, rows[2].ctypes.data_as(U64), cap, C.byref(n[2]), c["labels"].ctypes.data_as(U32), cells))
            t.append(time.perf_counter())
            rc.append(lib.kicp_grid_occupancy(h, 1, c["occ"].ctypes.data_as(C.POINTER(C.c_byte)), cells))
            middle = time.perf_counter()
            rc.append(lib.kicp_frontiers_from_occupancy(c["occ"].ctypes.data_as(C.POINTER(C.c_byte)), c["occ"].shape[1], c["occ"].shape[0], C.byref(cfg),
                                                        c["potential"].ctypes.data_as(U32), rows[3].ctypes.data_as(U64), cap, C.byref(n[3]), None, 0))
            t.append(time.perf_counter())
            if r == 0:
                assert rc == [0] * 5 and len({v.value for v in n}) == 1, (rc, [v.value for v in n])
                F = n[0].value
                assert np.array_equal(rows[1][:F], rows[3][:F]) and np.array_equal(rows[2][:F], rows[3][:F]) and np.array_equal(rows[0][:F, :8], rows[3][:F, :8])
                assert (rows[0][:F, 8] == K.UNREACHED).all() and np.array_equal(rows[0][:F, 9], rows[0][:F, 0])
                host_rows, host_labels = K.frontiers_from_occupancy(c["occ"], potential=c["potential"], return_labels=True)
                assert np.array_equal(host_labels, c["labels"]) and np.array_equal(host_rows, rows[3][:F])
                size = rows[3][:F, 1]
                c["result"] = {"frontiers": int(F), "frontier_cells": int(size.sum()), "largest_frontier": int(size.max()) if F else 0,
                               "reached_frontiers": int((rows[3][:F, 8] != K.UNREACHED).sum()), "frontiers_of_5_cells_or_more": int((size >= 5).sum())}
            if r >= 3:
                for k, name in enumerate(names[:4]):
                    c["t"][name].append((t[k + 1] - t[k]) * 1e3)
                c["t"]["host_alone"].append((t[4] - middle) * 1e3)
    out = []
    for c in todo:
        out.append({"scene": c["name"], "points": c["points"], "frames": a.frames, "cell_m": c["cell"], "grid_cells": [c["cfg"]["width"], c["cfg"]["height"]],
                    "robot_cell": list(c["start"]), **c["result"], "grid_frontiers_ms": spread(c["t"]["plain"]), "grid_frontiers_use_plan_ms": spread(c["t"]["use_plan"]),
                    "grid_frontiers_use_plan_labels_ms": spread(c["t"]["use_plan_labels"]), "host_occupancy_then_frontiers_ms": spread(c["t"]["host_route"]),
                    "host_frontiers_from_occupancy_alone_ms": spread(c["t"]["host_alone"])})
    print(json.dumps({"caller_process": where, "rounds": a.rounds, "frontiers": out}))


if __name__ == "__main__":
    main()
