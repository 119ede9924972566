"""The whole-map relocalisation through the drop-in C++ headers (tests/cpp/search_facade_test.cpp): KinematicICP::BuildOccupancy +
KinematicICP::RelocalizeSearch on a map loaded from a file, which must return - bit for bit - what the Python mirror returns for the
same keypoints, window and map, and whose result must become the pipeline's pose; KinematicRegistration::RelocalizeSearch likewise."""
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
from kinematic_icp_amd import synthetic as syn

CPP = os.path.join(ROOT, "kinematic_icp_amd", "cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "search_facade_test")


def build_binary():
    src = os.path.join(ROOT, "tests", "cpp", "search_facade_test.cpp")
    deps = [src] + [os.path.join(dp, f) for dp, _, fs in os.walk(CPP) for f in fs] + [os.path.join(ROOT, "include", "kicp.h")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        libdir = os.path.join(ROOT, "kinematic_icp_amd")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CPP, "-I", os.path.join(CPP, "compat"),
                               "-I", os.path.join(ROOT, "include"), src, "-o", BIN, "-L", libdir, "-lkicp_amd",
                               "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"])
    return BIN


def test_search_facade_compiles_and_links():
    assert os.path.exists(build_binary())


def _values(line):
    return np.array([float(x) for x in line.split()[1:]])


@pytest.mark.gpu
def test_relocalize_search_through_the_pipeline(tmp_path):
    # the scene of tests/test_planar_facade.py at the pipeline's default voxel size (1 m): a map of surface samples and one scan's
    # keypoints; the window spans 3 m x 3 m around a point 0.6 m off the truth, the full circle in 3 deg steps
    rng = np.random.Generator(np.random.PCG64(78))
    scene = syn.make_scene(rng, half=16.0, height=4.0, n_boxes=6, box_xy=(2.0, 5.0), box_z=(1.5, 3.5), keep_clear=3.0)
    dirs = syn.beam_directions(12, 512, (-20.0, 8.0))
    truth = syn.planar_pose(0.4, -0.3, 0.2)
    origin = truth[4:] + np.array([0.0, 0.0, 0.9])
    R = syn.quat_to_matrix(truth[:4])
    ranges = scene.raycast(origin, dirs @ R.T) + rng.normal(0, 0.01, len(dirs))
    frame = dirs * ranges[:, None] + np.array([0.0, 0.0, 0.9])  # base frame
    default = K.VoxelHashMap(1.0, 100.0, 20)  # pipeline::Config's defaults
    world = syn.pose_act(truth, frame)
    for _ in range(3):
        default.AddPoints(world + rng.normal(0, 0.01, world.shape))
    map_path = str(tmp_path / "map.pcd")
    default.save_pcd(map_path)
    keypoints = np.ascontiguousarray(frame[::7])
    cell, dilate, levels, top_m, max_iterations, convergence = 0.25, 1, 3, 6, 60, 1e-4  # (cell: about 1 m / sqrt(20))
    center, half, yaw_step = (0.9, 0.1), 1.5, np.deg2rad(3.0)
    f = tmp_path / "input.bin"
    with open(f, "wb") as fh:
        np.array([cell, dilate, levels, top_m, max_iterations, convergence, center[0], center[1], half, half, truth[6], yaw_step, len(keypoints)],
                 dtype=np.float64).tofile(fh)
        keypoints.tofile(fh)
    out = subprocess.check_output([build_binary(), map_path, str(f)], text=True).splitlines()
    line = lambda tag: [ln for ln in out if ln.split()[0] == tag][0]  # noqa: E731

    assert line("refused_without_pyramid").split()[1] == "1"
    gmap = K.VoxelHashMap.load_pcd(map_path, device=0)
    occ = K.OccupancyPyramid(gmap, cell, dilate, levels)
    info = occ.info()
    assert [int(v) for v in line("occupancy").split()[1:]] == info["dims"].tolist() + [info["set_cells"]]
    window = K.search_window_around(occ, center, half, half, truth[6], yaw_step)
    assert (window.nx, window.ny, window.nyaw) == (13, 13, 120)
    assert np.array_equal(_values(line("window")), [window.x0, window.y0, window.z, window.nx, window.ny, window.yaw0, window.yaw_step, window.nyaw])
    reg = K.KinematicRegistration()
    tau = 3.0 * (1.0 / np.sqrt(20) + 0.0)  # CorrespondenceThreshold::ComputeThreshold after Reset (no odometry error yet)
    pose, node, before, after = reg.RelocalizeSearch(keypoints, gmap, occ, window, tau, top_m=top_m, max_iterations=max_iterations, convergence=convergence)
    assert reg.last_status == K.KICP_OK
    for tag, pose_tag in (("relocalized", "relocalized_pose"), ("registration", "registration_pose")):
        assert np.array_equal(_values(line(pose_tag)), pose)
        got = line(tag).split()[1:]
        assert (int(got[0]), float(got[1]), float(got[2]), int(got[3])) == (node, before, after, 1)
    assert np.array_equal(_values(line("pose_after_relocalize")), pose)  # the result became the pipeline's pose
    err = syn.pose_mul(syn.pose_inverse(truth), pose)
    print("search facade: %.4f m, %.4f deg from the truth" % (np.hypot(err[4], err[5]), np.degrees(2 * abs(np.arcsin(err[2])))))
    assert np.hypot(err[4], err[5]) < cell and 2 * abs(np.arcsin(err[2])) < yaw_step  # within one cell and one yaw step
