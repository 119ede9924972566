"""The host side of the planar 3-DoF refinement, without a GPU: kicp_planar_step against the numpy restatement (tests/planar_ref.py),
the header it comes from in a stand-alone program under ASan + UBSan, and the recovery inputs of tests/test_gpu_planar.py pinned on
the CPU oracle alone.

Recovery: cfg1, both scans of make_case(..., n_scans=2), tau = first_frame_tau() and twice that; a 5 x 5 x 5 grid (0.5 m, 6 deg;
125 candidates) centred truth * planar(0.7, -0.4, 8.1 deg); the 8 cheapest refined by planar_ref.refine over okicp.associate with 100
iterations / convergence 1e-4, the cheapest refined pose taken.  Measured on the oracle: scan 0 ends 0.029 m / 0.045 deg from the truth,
scan 1 0.078 m / 0.043 deg, at both thresholds; 27 .. 83 iterations; the iteration started AT the truth ends at the same point
(differences <= 3e-12).  The kinematic refinement of kicp_relocalize ends 0.108 .. 0.110 m away on a 729-candidate grid
(tests/test_gpu_relocalize.py)."""
import functools
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from kinematic_icp_amd import synthetic as syn
from conftest import ROOT
from oracle import okicp
import planar_ref as pr

TOP_M = 8
END_POINT = [(0.029, 0.045), (0.078, 0.043)]  # per scan: distance [m], yaw [deg] of the best refined pose from the truth


def offset(truth, pose):
    """(distance [m], |yaw| [deg]) of a planar pose from the truth"""
    e = syn.pose_mul(syn.pose_inverse(truth), pose)
    return float(np.hypot(e[4], e[5])), float(np.degrees(2.0 * np.arcsin(min(1.0, abs(e[2])))))


def cost_of(n, n_corr, ssr, tau):
    return (ssr + (float(n) - n_corr) * (tau * tau)) / float(n)


@functools.lru_cache(maxsize=None)
def recovery_case():
    """the oracle's map, and per scan (keypoints, truth, the 125 candidates)"""
    cfg, scene, scans, rng = syn.make_case("cfg1", n_scans=2)
    omap = okicp.VoxelHashMap(cfg.voxel_size, cfg.max_range, cfg.max_points_per_voxel)
    syn.build_map_points(scene, cfg, omap.AddPoints, omap.num_points, rng)
    items = []
    for sc in scans:
        keypoints = okicp.voxel_downsample(okicp.voxel_downsample(sc["frame"], cfg.voxel_size * 0.5), cfg.voxel_size * 1.5)
        center = syn.pose_mul(sc["true_pose"], syn.planar_pose(0.7, -0.4, np.deg2rad(8.1)))
        grid = K.planar_grid(center, 1.0, 1.0, np.deg2rad(12.0), 0.5, 0.5, np.deg2rad(6.0))
        assert grid.shape == (125, 7)
        items.append((keypoints, sc["true_pose"], grid))
    return cfg, omap, items


def _random_rows(rng, count):
    """sums of random configurations: 3 .. 400 points within +-30 m, residual components within +-0.5 m.  A = J^T J of >= 3 random points
    has a condition number below ~1e4 (its eigenvalues lie between ~N and ~N 30^2 once the points spread), so a 3x3 solve in fp64
    agrees with another to condition x eps ~ 1e-12 relative."""
    rows = []
    while len(rows) < count:
        n = int(rng.integers(3, 400))
        s, r = rng.uniform(-30, 30, (n, 2)), rng.uniform(-0.5, 0.5, (n, 3))
        a, b = r[:, 0], r[:, 1]
        row = np.array([n, s[:, 0].sum(), s[:, 1].sum(), (s * s).sum(), a.sum(), b.sum(), (s[:, 0] * b - s[:, 1] * a).sum(), (r * r).sum()])
        A = np.array([[row[0], 0, -row[2]], [0, row[0], row[1]], [-row[2], row[1], row[3]]])
        if np.linalg.cond(A) < 1e4:
            rows.append(row)
    return rows


def test_planar_step_against_numpy():
    rng = np.random.default_rng(5)
    for row in _random_rows(rng, 200):
        # |t| < 8: the sum pose.t + R dx rounds at ulp(8) / 2 < 1e-15, the two evaluations of R dx differ by a few eps |dx|
        pose = syn.planar_pose(rng.uniform(-7, 7), rng.uniform(-7, 7), rng.uniform(-3, 3), z=rng.uniform(-1, 1))
        got = K.planar_step(row, pose)
        want_pose, want_dx = pr.solve_and_update(row, pose)
        assert got is not None
        np.testing.assert_allclose(got[1], want_dx, rtol=1e-12, atol=0)
        np.testing.assert_allclose(got[0], want_pose, rtol=0, atol=1e-14)


@pytest.mark.parametrize("row", [
    [0, 0, 0, 0, 0, 0, 0, 0], [1, 1.5, -2.0, 6.25, 0.1, 0.2, 0.7, 0.05], [5, 7.5, -10.0, 31.25, 0.5, 1.0, 3.5, 0.25],
    [3, np.nan, 1, 9, 0, 0, 0, 1], [3, 1, 1, 9, 0, 0, 0, np.nan], [np.nan, 1, 1, 9, 0, 0, 0, 1],
], ids=["no_correspondence", "one_point", "all_points_on_one_xy", "nan_sum", "nan_ssr", "nan_count"])
def test_degenerate_rows_leave_the_outputs_untouched(row):
    dp = K._dp
    sums, pose = np.array(row, dtype=np.float64), syn.planar_pose(1.0, 2.0, 0.3)
    out, dx = np.full(7, 42.0), np.full(3, 43.0)
    assert K.lib().kicp_planar_step(sums.ctypes.data_as(dp), pose.ctypes.data_as(dp), out.ctypes.data_as(dp), dx.ctypes.data_as(dp)) == 0
    assert (out == 42.0).all() and (dx == 43.0).all()
    assert K.planar_step(row, pose) is None and pr.solve_and_update(row, pose) is None


def test_zero_step_and_null_arguments():
    pose = syn.planar_pose(3.0, -4.0, 1.1, z=0.5)
    got_pose, dx = K.planar_step([4, 2.0, -1.0, 30.0, 0.0, 0.0, 0.0, 0.5], pose)
    assert not dx.any()
    np.testing.assert_allclose(got_pose, pose, rtol=0, atol=2.3e-16)  # (the product is re-normalised: an ulp of the quaternion)
    assert np.array_equal(got_pose[4:], pose[4:])
    dp = K._dp
    p = pose.ctypes.data_as(dp)
    assert K.lib().kicp_planar_step(None, p, p, None) == K.KICP_ERR_ARG
    assert K.lib().kicp_planar_step(p, None, p, None) == K.KICP_ERR_ARG
    assert K.lib().kicp_planar_step(p, p, None, None) == K.KICP_ERR_ARG


def test_planar_solve_stand_alone_under_sanitizers(tmp_path):
    """kicp_planar_host.hpp + kicp_se3.hpp in a program of their own (tests/cpp/planar_step_test.cpp), ASan + UBSan, as a subprocess"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    if not os.path.exists(os.path.join(include, "hip", "hip_runtime.h")):
        pytest.skip("the HIP headers kicp_se3.hpp declares its host / device functions with are not present")
    exe = str(tmp_path / "planar_step_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I", include, "-I", os.path.join(ROOT, "kinematic_icp_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "planar_step_test.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
    assert out.stdout.strip().startswith("ok "), out.stdout[-2000:]
    assert int(out.stdout.split()[1]) > 1000


def test_recovery_inputs_on_the_oracle_alone():
    """pins the inputs of the GPU recovery test: what planar_ref.refine over the oracle's DataAssociation reaches on them"""
    cfg, omap, items = recovery_case()
    for (keypoints, truth, grid), (dist, yaw_deg) in zip(items, END_POINT):
        n = len(keypoints)
        for tau in (cfg.first_frame_tau(), 2.0 * cfg.first_frame_tau()):
            def associate(pose):
                return okicp.associate(omap, keypoints, pose, tau)[:2]
            sums = np.array([okicp.icp_pass(omap, keypoints, g, tau)[0] for g in grid])
            order = np.argsort(cost_of(n, sums[:, 6], sums[:, 5], tau), kind="stable")
            best = None
            for j in order[:TOP_M]:
                pose, iterations, status = pr.refine(associate, keypoints, grid[j], 100, 1e-4)
                assert status == pr.CONVERGED and 17 <= iterations <= 83
                after = okicp.icp_pass(omap, keypoints, pose, tau)[0]
                c = cost_of(n, after[6], after[5], tau)
                if best is None or c < best[0]:
                    best = (c, pose)
            d, yaw = offset(truth, best[1])
            assert round(d, 3) == dist and round(yaw, 3) == yaw_deg, (d, yaw)
            assert d < 0.09 and yaw < 0.1  # the condition the GPU test asserts
            fixed, iterations, status = pr.refine(associate, keypoints, truth, 100, 1e-4)
            assert status == pr.CONVERGED
            np.testing.assert_allclose(fixed, best[1], rtol=0, atol=1e-9)
