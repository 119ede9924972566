"""Inputs shared by the occupancy grid's tests (tests/test_grid_host.py on the CPU, tests/test_gpu_grid.py on the GPU): seeded frames,
poses and configurations, so that the stand-alone host program and the kernels are held to the restatement on the same data."""
import numpy as np

import grid_ref as gr
from kinematic_icp_amd import synthetic as syn

IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def tilted_pose(x, y, yaw, roll, pitch, z=0.0):
    """yaw * pitch * roll as a unit quaternion + translation: a wheeled robot on a ramp or over a bump"""
    q = syn.quat_mul(np.array([0.0, 0.0, np.sin(yaw / 2), np.cos(yaw / 2)]),
                     syn.quat_mul(np.array([0.0, np.sin(pitch / 2), 0.0, np.cos(pitch / 2)]), np.array([np.sin(roll / 2), 0.0, 0.0, np.cos(roll / 2)])))
    return np.concatenate([q / np.linalg.norm(q), [x, y, z]])


def pinned_8x6():
    """Two returns seen from cell (0, 0) of an 8 x 6 grid of 1 m cells at the identity pose.  Expected, written out cell by cell
    (H hit, m miss, . untouched; row iy = 5 on top):
        iy 5   . . H . . . . .
        iy 4   . . m . . . . .
        iy 3   . m . . . . m H
        iy 2   . m . . m m . .
        iy 1   m . m m . . . .
        iy 0   m m . . . . . .
    first ray to (7, 3): a = 7, b = 3, m = 7, x = k, y = (6 k + 7) / 14 = 0 0 1 1 2 2 3 -> (0,0) (1,0) (2,1) (3,1) (4,2) (5,2) (6,3)
    second ray to (2, 5): a = 2, b = 5, m = 5, y = k, x = (4 k + 5) / 10 = 0 0 1 1 2   -> (0,0) (0,1) (1,2) (1,3) (2,4)"""
    cfg = gr.make_config(1.0, 0.0, 0.0, 8, 6, -1.0, 1.0, 8.0)
    points = np.array([[7.5, 3.5, 0.0], [2.5, 5.5, 0.5]])
    hit = {(7, 3), (2, 5)}
    miss = {(0, 0), (1, 0), (2, 1), (3, 1), (4, 2), (5, 2), (6, 3), (0, 1), (1, 2), (1, 3), (2, 4)}
    return cfg, points, IDENTITY, np.array([0.5, 0.5, 0.0]), hit, miss


def random_drive(seed=91, n=2000):
    """Six frames of n random points on a 200 x 160 grid of 0.1 m cells: roll and pitch of a few degrees, any yaw, two poses near the
    border so that the window is clipped; ranges beyond max_ray, heights outside the band and a few non-finite coordinates included"""
    cfg = gr.make_config(0.1, -10.0, -8.0, 200, 160, 0.1, 1.5, 6.0)
    rng = np.random.default_rng(seed)
    places = [(0.3, -0.2), (2.5, 1.0), (-4.0, 3.3), (6.1, -5.2), (-9.6, -7.7), (9.8, 7.6)]
    sensor = np.array([0.2, 0.0, 0.4])
    frames = []
    for x, y in places:
        pose = tilted_pose(x, y, rng.uniform(-np.pi, np.pi), np.deg2rad(rng.uniform(-4, 4)), np.deg2rad(rng.uniform(-4, 4)), z=rng.uniform(-0.05, 0.05))
        az, rng_m = rng.uniform(-np.pi, np.pi, n), rng.uniform(0.2, 8.0, n)
        pts = np.stack([sensor[0] + rng_m * np.cos(az), sensor[1] + rng_m * np.sin(az), rng.uniform(-0.2, 2.0, n)], axis=1)
        pts[rng.integers(0, n, 3), rng.integers(0, 3, 3)] = [np.nan, np.inf, -np.inf]
        frames.append((np.ascontiguousarray(pts), pose, sensor))
    return cfg, frames


def write_frames(path, cfg, frames):
    """the input file of tests/cpp/grid_host_test.cpp"""
    with open(path, "wb") as f:
        np.array([cfg["cell"], cfg["origin_x"], cfg["origin_y"], cfg["width"], cfg["height"], cfg["z_min"], cfg["z_max"], cfg["max_ray"], len(frames)],
                 dtype=np.float64).tofile(f)
        for pts, pose, sensor in frames:
            np.concatenate([np.asarray(pose, dtype=np.float64), np.asarray(sensor, dtype=np.float64), [float(len(pts))]]).tofile(f)
            np.ascontiguousarray(pts, dtype=np.float64).tofile(f)


def reference_run(cfg, frames):
    """-> (counts after every frame, stats of every frame) by the restatement"""
    counts = np.zeros((cfg["height"], cfg["width"], 2), dtype=np.uint16)
    after, stats = [], []
    for pts, pose, sensor in frames:
        stats.append(gr.integrate(cfg, counts, pts, pose, sensor))
        after.append(counts.copy())
    return after, stats
