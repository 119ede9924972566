"""Wall time of the whole-map relocalisation (kicp_occ_build, kicp_search_poses, kicp_relocalize_search), one process, the caller bound
as tools/bench_pipeline.py binds it.  Rows: cfg4's keypoints over its WHOLE map at 0.05 m / 1 deg, cfg1's over its whole map at
0.25 m / 2 deg (windows: kicp_search_window_around with half extents 0; z = the scan's true height).  Per row
  - the build of the occupancy pyramid;
  - kicp_search_poses with top_m = 8: time, nodes scored of nodes total, launches, and how far the best node lies from the truth;
  - kicp_relocalize_search (the search + the planar refinement of the eight finalists): time and how far its result lies from the truth;
  - next to them kicp_score_poses on a 65 536-pose sub-grid of the same window (64 x 64 positions x 16 yaws spread over it), and the
    time the WHOLE window would take at that rate - EXTRAPOLATED (nodes total / 65 536 x the measured time), never run.
Warm; the rows' calls alternate `rounds` times: median, p10 / p90, min .. max.  Prints one JSON line.

    python tools/bench_search.py [--rounds 5] [--top-m 8]
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
import kinematic_icp_amd as K  # noqa: E402
from kinematic_icp_amd import synthetic as syn  # noqa: E402
from bench_pipeline import placement  # noqa: E402
from bench_relocalize import offset, spread  # noqa: E402
from oracle import okicp  # noqa: E402  (the host-side voxel downsample that makes the keypoints; nothing of it is timed)

ROWS = (("cfg4", 0.05, 1.0, 6), ("cfg1", 0.25, 2.0, 5))  # config, cell [m], yaw step [deg], levels
DILATE = 1


def node_pose(window, cell, node):
    ix, row = int(node) % window.nx, int(node) // window.nx
    iy, j = row % window.ny, row // window.ny
    yaw = window.yaw0 + float(j) * window.yaw_step
    return np.array([0.0, 0.0, np.sin(0.5 * yaw), np.cos(0.5 * yaw), window.x0 + float(ix) * cell, window.y0 + float(iy) * cell, window.z])


def sub_grid(window, cell, per_axis=64, yaws=16):
    """per_axis x per_axis x yaws nodes spread evenly over the window, as poses"""
    ix = np.unique(np.linspace(0, window.nx - 1, per_axis).astype(np.int64))
    iy = np.unique(np.linspace(0, window.ny - 1, per_axis).astype(np.int64))
    jj = np.unique(np.linspace(0, window.nyaw - 1, yaws).astype(np.int64))
    j, y, x = np.meshgrid(jj, iy, ix, indexing="ij")
    nodes = ((j * window.ny + y) * window.nx + x).ravel()
    return np.ascontiguousarray(np.array([node_pose(window, cell, nd) for nd in nodes]))


def row(name, cell, yaw_deg, levels, rounds, top_m):
    cfg, scene, scans, rng = syn.make_case(name, n_scans=1)
    gmap = K.VoxelHashMap(cfg.voxel_size, cfg.max_range, cfg.max_points_per_voxel, device=0)
    syn.build_map_points(scene, cfg, gmap.AddPoints, gmap.num_points, rng)
    s = scans[0]
    truth = s["true_pose"]
    keypoints = np.ascontiguousarray(okicp.voxel_downsample(okicp.voxel_downsample(s["frame"], cfg.voxel_size * 0.5), cfg.voxel_size * 1.5))
    reg = K.KinematicRegistration()
    tau = cfg.first_frame_tau()
    gmap.sync(0)
    occ = K.OccupancyPyramid(gmap, cell, DILATE, levels)  # warm
    window = K.search_window_around(occ, None, 0.0, 0.0, truth[6], np.deg2rad(yaw_deg))
    poses = sub_grid(window, cell)
    times = {"build": [], "search": [], "relocalize_search": [], "score_poses_sub_grid": []}
    found = {}
    for r in range(rounds + 1):  # (the first round warms)
        t0 = time.perf_counter()
        occ = K.OccupancyPyramid(gmap, cell, DILATE, levels)
        t1 = time.perf_counter()
        nodes, hits, best = reg.SearchPoses(keypoints, occ, window, top_m)
        t2 = time.perf_counter()
        found["search"] = dict(offset(truth, best[0]), best_hits=int(hits[0]), nodes_scored=int(reg.get_option("search_nodes_scored")),
                               launches=int(reg.get_option("search_launches")))
        t3 = time.perf_counter()
        pose, node, before, after = reg.RelocalizeSearch(keypoints, gmap, occ, window, tau, top_m=top_m)
        t4 = time.perf_counter()
        found["relocalize_search"] = dict(offset(truth, pose), node=int(node), cost_before=before, cost_after=after, status=int(reg.last_status))
        reg.ScorePoses(keypoints, gmap, poses, tau)
        t5 = time.perf_counter()
        if r:
            for key, ms in (("build", t1 - t0), ("search", t2 - t1), ("relocalize_search", t4 - t3), ("score_poses_sub_grid", t5 - t4)):
                times[key].append(ms * 1e3)
    info = occ.info()
    total = window.nodes
    sub_ms = float(np.median(times["score_poses_sub_grid"]))
    search_ms = float(np.median(times["search"]))
    extrapolated_ms = sub_ms * total / len(poses)
    return {"scan": name, "keypoints": len(keypoints), "cell_m": cell, "yaw_step_deg": yaw_deg, "dilate": DILATE, "levels": levels,
            "grid_cells": info["dims"].tolist(), "set_cells": info["set_cells"], "pyramid_bytes": int(4 * occ.level(0).size * (levels + 1)),
            "window": [window.nx, window.ny, window.nyaw], "nodes_total": total,
            "build": spread(times["build"]), "search_top%d" % top_m: dict(spread(times["search"]), **found["search"]),
            "relocalize_search_top%d" % top_m: dict(spread(times["relocalize_search"]), **found["relocalize_search"]),
            "score_poses_sub_grid": dict(spread(times["score_poses_sub_grid"]), poses=len(poses), queries_per_s=len(poses) * len(keypoints) / (sub_ms * 1e-3)),
            "score_poses_whole_window_EXTRAPOLATED_ms": extrapolated_ms,
            "search_vs_extrapolated_exhaustive": extrapolated_ms / search_ms,
            "search_beats_extrapolated_exhaustive": bool(search_ms < extrapolated_ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--top-m", type=int, default=8)
    ap.add_argument("--rows", default="cfg4,cfg1")
    a = ap.parse_args()
    bind, where = placement()
    if bind:
        bind()
    res = {"caller_process": where, "rounds": a.rounds, "rows": []}
    for name, cell, yaw_deg, levels in ROWS:
        if name in a.rows.split(","):
            res["rows"].append(row(name, cell, yaw_deg, levels, a.rounds, a.top_m))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
