"""What see-through removal costs per frame (kicp_view_*, kicp_map_remove_seen_through), one process, the caller bound as
tools/bench_pipeline.py binds it.

Cases: a 131 072-point frame (64 beams x 2048 azimuths) ray-cast in cfg1's scene against a cfg1-sized map (100 000 points) and in cfg2's
scene against a cfg2-sized map (about 1 000 000 points), each at res 128, 256 and 512 (window 2, min_rays 2, 0.2 m + 0.02 m per metre).
Per case
  - kicp_view_render_device (the frame already in HBM: what the pipeline calls), kicp_map_remove_seen_through, and both in a row: the
    host clock around the calls, which return after their kernels have completed.  Warm; the cases' calls alternate `rounds` times;
    median, p10 / p90, min .. max.  The first sweep of a map removes what the frame sees through; the timed ones find a swept map, which is
    what a frame of a drive meets - their statistics are reported beside the first sweep's;
  - with --pipeline: KinematicICP::RegisterFrame on a short drive in cfg1's scene (tests/cpp/view_facade_test, mode `timed`; the frames
    as vectors, the clock around the call), a process with the removal and a process without, alternating `pipeline-rounds` times: the
    median of the drive's second half per process, then median and min .. max over the processes.
Prints one JSON line.

    python tools/bench_view.py [--rounds 30] [--maps cfg1,cfg2] [--pipeline] [--pipeline-rounds 3] [--pipeline-frames 16]
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

BEAMS, AZIMUTHS = 64, 2048
RESOLUTIONS = (128, 256, 512)
WINDOW, MIN_RAYS, MAX_RAY, MARGIN, MARGIN_PER_METRE = 2, 2, 60.0, 0.2, 0.02


def make_view(res):
    return K.DepthView(res, WINDOW, MIN_RAYS, MAX_RAY, MARGIN, MARGIN_PER_METRE)


def sweep_rows(rounds, maps):
    cases = []
    for name in maps:
        cfg = syn.CONFIGS[name]
        rng = np.random.Generator(np.random.PCG64(cfg.seed))
        scene = syn.make_scene(rng, **cfg.scene_kw)
        dirs = syn.beam_directions(BEAMS, AZIMUTHS, cfg.elev_deg, cfg.az_span_deg)
        pose = syn.planar_pose(1.2, -0.7, 0.9)
        frame = np.ascontiguousarray(syn.make_scan(scene, pose, dirs, cfg.sensor_height, rng))
        sensor = np.array([0.0, 0.0, cfg.sensor_height])
        samples = scene.sample_surface(int(cfg.map_points * 1.6), rng)
        for res in RESOLUTIONS:
            gmap = K.VoxelHashMap(cfg.voxel_size, cfg.max_range, cfg.max_points_per_voxel, device=0)
            gmap.AddPoints(samples)
            gmap.sync(0)
            view = make_view(res)
            dev = K.DeviceFrame(frame)
            before = (gmap.num_points(), gmap.num_voxels())
            used = view.render_device(dev, pose, sensor)
            first = gmap.RemoveSeenThrough(view)
            cases.append(dict(name=name, res=res, map=gmap, view=view, dev=dev, pose=pose, sensor=sensor, before=before, used=used, first=first, n=len(frame),
                              t_render=[], t_sweep=[], t_both=[]))
    for r in range(rounds + 3):  # (the first three rounds warm)
        for c in cases:
            t0 = time.perf_counter()
            c["view"].render_device(c["dev"], c["pose"], c["sensor"])
            t1 = time.perf_counter()
            c["steady"] = c["map"].RemoveSeenThrough(c["view"])
            t2 = time.perf_counter()
            c["view"].render_device(c["dev"], c["pose"], c["sensor"])
            c["map"].RemoveSeenThrough(c["view"])
            t3 = time.perf_counter()
            if r >= 3:
                c["t_render"].append((t1 - t0) * 1e3), c["t_sweep"].append((t2 - t1) * 1e3), c["t_both"].append((t3 - t2) * 1e3)
    rows = []
    for c in cases:
        rows.append({"map": c["name"], "frame_points": c["n"], "res": c["res"], "map_points": c["before"][0], "map_voxels": c["before"][1], "points_used": c["used"][0],
                     "first_sweep": dict(zip(("in_range", "removed", "voxels_touched", "voxels_erased"), c["first"])),
                     "steady_sweep": dict(zip(("in_range", "removed", "voxels_touched", "voxels_erased"), c["steady"])),
                     "render_device_ms": spread(c["t_render"]), "remove_seen_through_ms": spread(c["t_sweep"]), "both_ms": spread(c["t_both"])})
    return rows


def pipeline_rows(rounds, n_frames):
    import test_view_facade
    exe = test_view_facade.build_binary()
    bind, _ = placement()
    rows = []
    cfg = syn.CONFIGS["cfg1"]
    rng = np.random.Generator(np.random.PCG64(cfg.seed))
    scene = syn.make_scene(rng, **cfg.scene_kw)
    dirs = syn.beam_directions(BEAMS, AZIMUTHS, cfg.elev_deg, cfg.az_span_deg)
    with tempfile.TemporaryDirectory() as td:
        ext = np.concatenate([[0, 0, np.sin(0.05), np.cos(0.05)], [0.3, 0.0, cfg.sensor_height]])
        poses, drive = [syn.planar_pose(0.0, 0.0, 0.1)], os.path.join(td, "drive.bin")
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
        for res in RESOLUTIONS:
            vfile = os.path.join(td, "view.bin")
            np.array([res, WINDOW, MIN_RAYS, MAX_RAY, MARGIN, MARGIN_PER_METRE], dtype=np.float64).tofile(vfile)
            per, removed = {"on": [], "off": []}, None
            for r in range(rounds + 1):  # (the first pair warms the file cache and the driver)
                for which in ("off", "on"):
                    out = subprocess.check_output([exe, "timed", drive, vfile, which], text=True, preexec_fn=bind).splitlines()
                    ms = np.array([float(ln.split()[3]) for ln in out if ln.startswith("frame ")])
                    if which == "on":
                        removed = int([ln for ln in out if ln.startswith("points_removed ")][0].split()[1])
                    if r:
                        per[which].append(float(np.median(ms[len(ms) // 2:])))
            rows.append({"scene": "cfg1", "points": len(dirs), "res": res, "frames": n_frames, "points_removed_over_the_drive": removed,
                         "register_frame_ms_removal_off": spread(per["off"]), "register_frame_ms_removal_on": spread(per["on"]),
                         "what": "median RegisterFrame wall time of the drive's second half per process; spread over %d alternating processes each" % rounds})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--maps", default="cfg1,cfg2")
    ap.add_argument("--pipeline", action="store_true")
    ap.add_argument("--pipeline-rounds", type=int, default=3)
    ap.add_argument("--pipeline-frames", type=int, default=16)
    a = ap.parse_args()
    bind, where = placement()
    if bind:
        bind()
    res = {"caller_process": where, "rounds": a.rounds, "sweep": sweep_rows(a.rounds, [m for m in a.maps.split(",") if m])}
    if a.pipeline:
        res["pipeline"] = pipeline_rows(a.pipeline_rounds, a.pipeline_frames)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
