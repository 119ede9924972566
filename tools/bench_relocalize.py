"""Wall time of scoring one keypoint scan at many candidate poses (global localisation in a saved map), one process, the caller bound
as tools/bench_pipeline.py binds it.  For (cfg1 keypoints, 4 096 and 65 536 poses) and (cfg4 keypoints, 4 096 poses):
  (a) one kicp_score_poses_device call (the frame resident in HBM);
  (b) the way without it: a loop of kicp_pass_sums over the same poses, through bare ctypes calls with every pointer prepared
      beforehand (for 65 536 poses 4 096 of them are timed and the time is scaled by 16 - the JSON says so);
  (c) kicp_relocalize with top_m = 8 on the same candidates;
  (d) kicp_relocalize_planar (100 iterations, convergence 1e-4) on the same candidates;
  (e) kicp_relocalize_planar on a coarser grid over the same extent with about a sixth as many candidates (0.55 of the nodes per axis).
Warm; (a) and (b) alternate three times, then (c), (d) and (e) alternate as often: median, p10 / p90 and spread (min .. max), the
speed-up of the medians, and whether (a) beats (b) by more than both spreads.  Per row of (c) - (e) also how far the result lies from
the scan's true pose, and for (d) / (e) the launches of the call (scoring + one per lock-step iteration + scoring).  Also queries
(pose x point pairs) per second of (a).  Prints one JSON line.

    python tools/bench_relocalize.py [--rounds 3] [--top-m 8]
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
import kinematic_icp_amd as K  # noqa: E402
from kinematic_icp_amd import synthetic as syn  # noqa: E402
from bench_pipeline import placement  # noqa: E402
from oracle import okicp  # noqa: E402  (the host-side voxel downsample that makes the keypoints; nothing of it is timed)


def candidates(truth, nx, ny, nw, half_xy=2.0, half_yaw=np.deg2rad(20.0)):
    """nx x ny x nw planar poses around the (planar) truth, body-frame offsets, x slowest, yaw fastest"""
    yaw0 = 2.0 * np.arctan2(truth[2], truth[3])
    dx, dy, dw = np.meshgrid(np.linspace(-half_xy, half_xy, nx), np.linspace(-half_xy, half_xy, ny), np.linspace(-half_yaw, half_yaw, nw), indexing="ij")
    dx, dy, yaw = dx.ravel(), dy.ravel(), yaw0 + dw.ravel()
    out = np.zeros((len(dx), 7))
    out[:, 2], out[:, 3] = np.sin(yaw / 2), np.cos(yaw / 2)
    out[:, 4] = truth[4] + np.cos(yaw0) * dx - np.sin(yaw0) * dy
    out[:, 5] = truth[5] + np.sin(yaw0) * dx + np.cos(yaw0) * dy
    out[:, 6] = truth[6]
    return np.ascontiguousarray(out)


def spread(v):
    return {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v)), "p10_ms": float(np.percentile(v, 10)),
            "p90_ms": float(np.percentile(v, 90))}


def offset(truth, pose):
    """(distance [m], |yaw| [deg]) of a planar pose from the truth"""
    e = syn.pose_mul(syn.pose_inverse(truth), pose)
    return {"distance_m": float(np.hypot(e[4], e[5])), "yaw_deg": float(np.degrees(2.0 * np.arcsin(min(1.0, abs(e[2])))))}


def shape(name, cfg, gmap, keypoints, poses, coarse, truth, timed_b, rounds, top_m):
    lib, dp = K.lib(), C.POINTER(C.c_double)
    reg = K.KinematicRegistration()
    tau = cfg.first_frame_tau()
    n, count = len(keypoints), len(poses)
    dev = K.DeviceFrame(keypoints)
    frame_p, poses_p = keypoints.ctypes.data_as(dp), poses.ctypes.data_as(dp)
    n_corr, ssr, sums = np.zeros(count), np.zeros(count), np.zeros(7)
    n_p, s_p, sums_p = n_corr.ctypes.data_as(dp), ssr.ctypes.data_as(dp), sums.ctypes.data_as(dp)
    pose_ps = [C.cast(poses.ctypes.data + 56 * k, dp) for k in range(timed_b)]

    def a():
        t0 = time.perf_counter()
        rc = lib.kicp_score_poses_device(reg._h, gmap._h, dev.ptr, n, poses_p, count, tau, n_p, s_p)
        t1 = time.perf_counter()
        assert rc == 0, rc
        return (t1 - t0) * 1e3

    def b():
        first = np.zeros((timed_b, 2))
        t0 = time.perf_counter()
        for k in range(timed_b):
            lib.kicp_pass_sums(reg._h, gmap._h, frame_p, n, pose_ps[k], tau, sums_p)
            first[k] = sums[6], sums[5]
        t1 = time.perf_counter()
        return (t1 - t0) * 1e3 * (count / timed_b), first

    a(), b()  # warm: buffers, the map's HBM copy, code objects
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(a())
        ms, first = b()
        tb.append(ms)
        assert np.array_equal(first[:, 0], n_corr[:timed_b]) and np.array_equal(first[:, 1], ssr[:timed_b])  # the same doubles
    launches = int(reg.get_option("score_launches"))
    pose, cand = np.zeros(7), C.c_size_t()
    before, after = C.c_double(), C.c_double()
    coarse_p = coarse.ctypes.data_as(dp)
    rows = {"c": [], "d": [], "e": []}
    found = {}

    def relocalize(row):
        t0 = time.perf_counter()
        if row == "c":
            rc = lib.kicp_relocalize(reg._h, gmap._h, frame_p, n, poses_p, count, tau, top_m, pose.ctypes.data_as(dp), C.byref(cand), C.byref(before), C.byref(after))
        else:
            rc = lib.kicp_relocalize_planar(reg._h, gmap._h, frame_p, n, poses_p if row == "d" else coarse_p, count if row == "d" else len(coarse), tau, top_m,
                                            100, 1e-4, pose.ctypes.data_as(dp), C.byref(cand), C.byref(before), C.byref(after))
        rows[row].append((time.perf_counter() - t0) * 1e3)
        assert rc >= 0, rc
        found[row] = dict(offset(truth, pose), candidate=int(cand.value), cost_before=before.value, cost_after=after.value,
                          launches=int(reg.get_option("score_launches")))

    for _ in range(rounds + 1):  # (the first round warms)
        for row in ("c", "d", "e"):
            relocalize(row)
    tc = rows["c"]
    med_a, med_b = float(np.median(ta)), float(np.median(tb))
    return {"scan": name, "keypoints": n, "poses": count, "queries": n * count, "launches": launches,
            "score_poses": spread(ta), "pass_sums_loop": dict(spread(tb), timed_poses=timed_b, scaled_by=count / timed_b),
            "relocalize_top%d" % top_m: dict(spread(tc[1:]), **found["c"]),
            "relocalize_planar_top%d" % top_m: dict(spread(rows["d"][1:]), **found["d"]),
            "relocalize_planar_coarse_top%d" % top_m: dict(spread(rows["e"][1:]), poses=len(coarse), **found["e"]), "speedup_of_medians": med_b / med_a,
            "beats_by_more_than_the_spreads": bool(min(tb) - max(ta) > max(max(ta) - min(ta), max(tb) - min(tb))),
            "score_poses_queries_per_s": n * count / (med_a * 1e-3), "relocalized_candidate": found["c"]["candidate"], "cost_before": found["c"]["cost_before"],
            "cost_after": found["c"]["cost_after"], "best_candidate_correspondences": float(n_corr.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--top-m", type=int, default=8)
    a = ap.parse_args()
    bind, where = placement()
    if bind:
        bind()
    res = {"caller_process": where, "shapes": []}
    for name, grids in (("cfg1", ((16, 16, 16), (64, 32, 32))), ("cfg4", ((16, 16, 16),))):
        cfg, scene, scans, rng = syn.make_case(name, n_scans=1)
        gmap = K.VoxelHashMap(cfg.voxel_size, cfg.max_range, cfg.max_points_per_voxel, device=0)
        syn.build_map_points(scene, cfg, gmap.AddPoints, gmap.num_points, rng)
        s = scans[0]
        keypoints = np.ascontiguousarray(okicp.voxel_downsample(okicp.voxel_downsample(s["frame"], cfg.voxel_size * 0.5), cfg.voxel_size * 1.5))
        for nx, ny, nw in grids:
            poses = candidates(s["true_pose"], nx, ny, nw)
            # 0.55 of the nodes per axis (0.55^3 ~ 1 / 6), an even number of them in x and y: the truth stays between the nodes
            cx, cy, cw = (int(round(0.55 * k)) for k in (nx, ny, nw))
            coarse = candidates(s["true_pose"], cx - cx % 2, cy + cy % 2, cw)
            res["shapes"].append(shape(name, cfg, gmap, keypoints, poses, coarse, s["true_pose"], min(len(poses), 4096), a.rounds, a.top_m))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
