"""What the occupancy grid costs per frame (kicp_grid_*), one process, the caller bound as tools/bench_pipeline.py binds it.

Cases: a 131 072-point frame (64 beams x 2048 azimuths) in cfg1's scene and a 1 080-beam scan in cfg4's, each at 0.05 m and 0.25 m cells.
Per case
  - kicp_grid_integrate_device (the frame already in HBM: what the pipeline calls) and kicp_grid_integrate (the frame from host memory):
    the host clock around the call, which returns after its kernels have completed.  Warm; the cases' calls alternate `rounds` times;
    median, p10 / p90, min .. max;
  - what the frame was: points used, endpoint cells (HIT), carved cells (MISS), cell visits of the ray walk (the sum of the rays'
    lengths over the endpoint cells, from the numpy restatement), and the cells of the window the apply pass reads;
  - with --pipeline: KinematicICP::RegisterFrame on a short drive in the case's scene (tests/cpp/grid_facade_test, mode `timed`; the
    frames as vectors, the clock around the call), a process with the grid and a process without, alternating `pipeline-rounds` times:
    the median of the drive's second half per process, then median and min .. max over the processes.
Prints one JSON line.

    python tools/bench_grid.py [--rounds 30] [--pipeline] [--pipeline-rounds 3] [--pipeline-frames 16]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kinematic_icp_amd as K  # noqa: E402
from kinematic_icp_amd import synthetic as syn  # noqa: E402
from bench_pipeline import placement  # noqa: E402
from bench_relocalize import spread  # noqa: E402
import grid_ref as gr  # noqa: E402

# scene config, beams, azimuths, band (base frame), max_ray, half extent of the grid
GEOMETRY = {"cfg1": (64, 2048, (0.2, 2.2), 45.0, 40.0), "cfg4": (1, 1080, (0.1, 1.0), 25.0, 24.0)}
CELLS = (0.05, 0.25)


def grid_config(name, cell):
    _, _, (z_min, z_max), max_ray, half = GEOMETRY[name]
    side = int(round(2.0 * half / cell))
    return gr.make_config(cell, -half, -half, side, side, z_min, z_max, max_ray)


def make_grid(cfg):
    return K.OccupancyGrid(cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], cfg["z_min"], cfg["z_max"], cfg["max_ray"])


def scene_and_beams(name):
    cfg = syn.CONFIGS[name]
    rng = np.random.Generator(np.random.PCG64(cfg.seed))
    beams, az = GEOMETRY[name][:2]
    return cfg, syn.make_scene(rng, **cfg.scene_kw), syn.beam_directions(beams, az, cfg.elev_deg, cfg.az_span_deg), rng


def integrate_rows(rounds):
    cases = []
    for name in GEOMETRY:
        cfg, scene, dirs, rng = scene_and_beams(name)
        pose = syn.planar_pose(1.2, -0.7, 0.9)
        frame = np.ascontiguousarray(syn.make_scan(scene, pose, dirs, cfg.sensor_height, rng))
        sensor = np.array([0.0, 0.0, cfg.sensor_height])
        for cell in CELLS:
            gcfg = grid_config(name, cell)
            _, offs, _ = gr.endpoints(gcfg, frame, pose, sensor)
            visits = int(np.abs(np.unique(offs, axis=0)).max(axis=1).sum())
            cases.append(dict(name=name, cell=cell, cfg=gcfg, grid=make_grid(gcfg), frame=frame, dev=K.DeviceFrame(frame), pose=pose, sensor=sensor, visits=visits,
                              t_dev=[], t_host=[]))
    for r in range(rounds + 3):  # (the first three rounds warm)
        for c in cases:
            t0 = time.perf_counter()
            c["grid"].integrate_device(c["dev"], c["pose"], c["sensor"])
            t1 = time.perf_counter()
            c["stats"] = c["grid"].integrate(c["frame"], c["pose"], c["sensor"])
            t2 = time.perf_counter()
            if r >= 3:
                c["t_dev"].append((t1 - t0) * 1e3), c["t_host"].append((t2 - t1) * 1e3)
    rows = []
    for c in cases:
        side = 2 * c["cfg"]["reach"] + 1
        rows.append({"scene": c["name"], "points": len(c["frame"]), "cell_m": c["cell"], "grid_cells": [c["cfg"]["width"], c["cfg"]["height"]], "reach_cells": c["cfg"]["reach"],
                     "window_cells": side * side, "points_used": c["stats"][0], "cells_hit": c["stats"][2], "cells_miss": c["stats"][3], "ray_cell_visits": c["visits"],
                     "integrate_device_ms": spread(c["t_dev"]), "integrate_host_frame_ms": spread(c["t_host"])})
    return rows


def pipeline_rows(rounds, n_frames):
    import test_grid_facade
    exe = test_grid_facade.build_binary()
    bind, _ = placement()
    rows = []
    with tempfile.TemporaryDirectory() as td:
        for name in GEOMETRY:
            cfg, scene, dirs, rng = scene_and_beams(name)
            ext = np.concatenate([[0, 0, np.sin(0.05), np.cos(0.05)], [0.3, 0.0, cfg.sensor_height]])
            poses, drive = [syn.planar_pose(0.0, 0.0, 0.1)], os.path.join(td, name + ".bin")
            with open(drive, "wb") as fh:
                np.array([n_frames, cfg.voxel_size, cfg.max_range, 1.0]).tofile(fh)
                ext.tofile(fh)
                for k in range(n_frames):
                    delta_true = syn.planar_pose(0.2, 0.0, np.deg2rad(1.0 + 0.1 * k))
                    poses.append(syn.pose_mul(poses[-1], delta_true))
                    wl = syn.pose_mul(poses[-1], ext)
                    t = scene.raycast(wl[4:], dirs @ syn.quat_to_matrix(wl[:4]).T) + rng.normal(0, 0.01, len(dirs))
                    np.array([float(len(dirs))]).tofile(fh)
                    np.ascontiguousarray((dirs * t[:, None]).astype(np.float32).astype(np.float64)).tofile(fh)
                    np.linspace(0.0, 1.0, len(dirs)).astype(np.float32).astype(np.float64).tofile(fh)
                    syn.pose_mul(delta_true, syn.planar_pose(0.01 * (-1) ** k, 0.0, np.deg2rad(0.1))).tofile(fh)
            for cell in CELLS:
                gcfg = grid_config(name, cell)
                gfile = os.path.join(td, "grid.bin")
                np.array([gcfg[k] for k in ("cell", "origin_x", "origin_y", "width", "height", "z_min", "z_max", "max_ray")], dtype=np.float64).tofile(gfile)
                per = {"on": [], "off": []}
                for r in range(rounds + 1):  # (the first pair warms the file cache and the driver)
                    for which in ("off", "on"):
                        out = subprocess.check_output([exe, "timed", drive, gfile, which], text=True, preexec_fn=bind).splitlines()
                        ms = np.array([float(ln.split()[3]) for ln in out if ln.startswith("frame ")])
                        assert ("frames_integrated %d" % (n_frames if which == "on" else 0)) in out
                        if r:
                            per[which].append(float(np.median(ms[len(ms) // 2:])))
                rows.append({"scene": name, "points": len(dirs), "cell_m": cell, "frames": n_frames,
                             "register_frame_ms_grid_off": spread(per["off"]), "register_frame_ms_grid_on": spread(per["on"]),
                             "what": "median RegisterFrame wall time of the drive's second half per process; spread over %d alternating processes each" % rounds})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--pipeline", action="store_true")
    ap.add_argument("--pipeline-rounds", type=int, default=3)
    ap.add_argument("--pipeline-frames", type=int, default=16)
    a = ap.parse_args()
    bind, where = placement()
    if bind:
        bind()
    res = {"caller_process": where, "rounds": a.rounds, "integrate": integrate_rows(a.rounds)}
    if a.pipeline:
        res["pipeline"] = pipeline_rows(a.pipeline_rounds, a.pipeline_frames)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
