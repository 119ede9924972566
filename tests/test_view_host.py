"""The depth view without a GPU: the numpy restatement (tests/view_ref.py) against verdicts and pixels written out by hand, its
properties, the pinned 8-frame drive with a person walking through, and view_host::render / classify / sweep with
HostMap::RemovePointsIf - the host restatement over the very geometry and verdict the kernels call (kicp_view_host.hpp) - in a
stand-alone program, built plainly and under ASan + UBSan, against the restatement on the cases the GPU tests give the kernels."""
import os
import subprocess

import numpy as np
import pytest

from checkers import okicp
from conftest import ROOT
from mapdev_ref import bucket_sorted
import view_cases as vc
import view_ref as vr

UNIT = vc.unit_cases()
SWEEPS = vc.sweep_cases()


@pytest.mark.parametrize("name", sorted(UNIT))
def test_unit_case_of_the_restatement(name):
    """the restatement gives the pixels, statistics and verdicts that the case states by hand"""
    case = UNIT[name]
    depth, stats, c = vr.render(case["cfg"], case["frame"], case["pose"], case["sensor"])
    if case["stats"] is not None:
        assert stats == case["stats"]
    if case["pixels"] is not None:
        want = np.full_like(depth, np.inf)
        for (face, w_, u), d in case["pixels"].items():
            want[face, w_, u] = np.float32(d)
        assert np.array_equal(depth, want), sorted(zip(*np.nonzero(np.isfinite(depth))))
    if case["verdicts"] is not None:
        assert vr.verdict(case["cfg"], depth, c, case["queries"]).tolist() == case["verdicts"]
    assert stats[0] + stats[1] == len(case["frame"])


def test_image_does_not_depend_on_the_order_of_the_points():
    rng = np.random.default_rng(3)
    for name in ("contended", "tilted", "min_wins"):
        case = UNIT[name]
        depth, stats, _ = vr.render(case["cfg"], case["frame"], case["pose"], case["sensor"])
        for _ in range(3):
            again, stats2, _ = vr.render(case["cfg"], case["frame"][rng.permutation(len(case["frame"]))], case["pose"], case["sensor"])
            assert np.array_equal(depth, again) and stats == stats2
    contended = vr.render(UNIT["contended"]["cfg"], UNIT["contended"]["frame"], vc.IDENTITY, vc.ORIGIN)[0]
    assert np.isfinite(contended).sum() == 3


def test_pixel_border_hit_exactly():
    """binary-exact coordinates under the identity pose: a / m = k / 8 sits exactly on the border between pixels k + 7 and k + 8 at res 16
    and belongs to the upper one; 2^-40 below it (a step that survives the + 1.0) belongs to the lower one"""
    cfg = vr.make_config(16, 0, 1, 100.0, 0.0, 0.0)
    for k in range(-7, 8):
        ok, m, face, u, w = vr.project(cfg, np.array([[8.0, float(k), float(k) - 2.0 ** -37]]))
        assert ok[0] and m[0] == 8.0 and face[0] == 0 and u[0] == k + 8 and w[0] == k + 7
    ok, m, face, u, w = vr.project(cfg, np.array([[8.0, 8.0, -8.0], [-8.0, 8.0, 8.0], [0.5, -8.0, 8.0]]))
    assert face.tolist() == [0, 1, 3] and u.tolist() == [15, 15, 8] and w.tolist() == [0, 15, 15]


@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_sweep_case_loses_the_points_it_was_built_to_lose(name):
    case = SWEEPS[name]
    omap = okicp.VoxelHashMap(case["vs"], 100.0, case["cap"])
    omap.AddPoints(case["points"])
    assert omap.num_points() == len(case["points"])  # every point was accepted: the buckets hold them in insertion order
    depth, _, c = vr.render(vc.WALL_CFG, vc.wall(), vc.IDENTITY, vc.ORIGIN)
    assert np.all(depth[np.isfinite(depth)] == np.float32(10.5))
    v = vr.verdict(vc.WALL_CFG, depth, c, case["points"])
    assert np.array_equal((v & vr.SEEN_THROUGH) != 0, case["pattern"])
    keep, stats = vr.sweep(vc.WALL_CFG, depth, c, bucket_sorted(omap.Pointcloud(), case["vs"]), case["vs"])
    assert stats[1] == int(case["pattern"].sum()) and stats[0] == int(((v & vr.IN_RANGE) != 0).sum())
    if name == "full_bucket_erased":
        assert stats == (len(case["points"]) - 1, 22, 2, 1)  # the point at x = 40.5 is out of range


def test_pinned_drive_meets_its_conditions():
    """8 frames of 20 x 1000 beams through cfg1's scene, a 150-point person crossing; res 128, window 2, min_rays 2, 0.2 + 0.02 m, max_ray 60.
    Caps, not measurements: at most 1 % of the final map's static points removed over the whole drive, at least 90 % of the person's stale
    points gone, every person point of the last frame still there - also after a sweep with the last frame's own view."""
    d = vc.reference_drive()
    frames, final, plain = d["frames"], d["final"], d["plain"]
    past, last = range(len(frames) - 1), [len(frames) - 1]
    stale_plain, stale = vc.person_count(plain, frames, past), vc.person_count(final, frames, past)
    removed = np.concatenate([s["removed"] for s in d["steps"]])
    static_removed = len(removed) - vc.person_count(removed, frames, past)
    static_final = len(plain) - vc.person_count(plain, frames, range(len(frames)))
    print("drive: stale person points %d without removal, %d with; static points removed %d of %d; map %d points" %
          (stale_plain, stale, static_removed, static_final, len(final)))
    assert stale_plain >= 50  # the person does leave a trail
    assert static_removed <= 0.01 * static_final
    assert stale <= 0.10 * stale_plain
    last_there = vc.person_count(final, frames, last)
    assert last_there > 0 and last_there == vc.person_count(plain, frames, last)
    assert vc.person_count(final[d["self_keep"]], frames, last) == last_there
    assert all(s["sweep_stats"][1] == len(s["removed"]) for s in d["steps"])


def _build(tmp_path, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", include, "-I",
                           os.path.join(ROOT, "kinematic_icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "view_host_test.cpp"), "-o", exe] + extra)
    return exe


@pytest.fixture(scope="module")
def host_cases():
    """(cfg, vs, cap, map points, frame, pose, sensor, queries) per case: every unit case with a small random map around it, every sweep
    case behind the wall, and frame 3 of the drive over the map the drive has built by then"""
    rng = np.random.default_rng(17)
    cases = []
    for name in sorted(UNIT):
        c = UNIT[name]
        cases.append((c["cfg"], 0.5, 20, np.concatenate([c["queries"][np.all(np.isfinite(c["queries"]), axis=1)], rng.uniform(-6, 6, (300, 3))]), c["frame"], c["pose"], c["sensor"], c["queries"]))
    for name in sorted(SWEEPS):
        c = SWEEPS[name]
        cases.append((vc.WALL_CFG, c["vs"], c["cap"], c["points"], vc.wall(), vc.IDENTITY, vc.ORIGIN, c["points"]))
    d = vc.reference_drive()
    fr = d["frames"][3]
    cases.append((vc.DRIVE_CFG, vc.DRIVE_VS, vc.DRIVE_CAP, d["steps"][2]["after_update"], fr["frame"], fr["pose"], fr["sensor"], d["steps"][2]["after_update"][::7]))
    return cases


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_view_host_stand_alone(tmp_path, host_cases, flags):
    """view_host::render / classify / sweep in a program of its own (tests/cpp/view_host_test.cpp), as a subprocess; the sanitizers run on
    this host program only"""
    exe = _build(tmp_path, "view_host_test", flags)
    removed_somewhere = 0
    for k, (cfg, vs, cap, map_points, frame, pose, sensor, queries) in enumerate(host_cases):
        src, dst = str(tmp_path / ("in%d.bin" % k)), str(tmp_path / ("out%d.bin" % k))
        vc.write_host_case(src, cfg, vs, 100.0, cap, map_points, frame, pose, sensor, queries)
        out = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
        lines = {ln.split()[0]: tuple(int(v) for v in ln.split()[1:]) for ln in out.stdout.splitlines()}
        omap = okicp.VoxelHashMap(vs, 100.0, cap)
        omap.AddPoints(map_points)
        before = bucket_sorted(omap.Pointcloud(), vs)
        depth, rstats, c = vr.render(cfg, frame, pose, sensor)
        keep, sstats = vr.sweep(cfg, depth, c, before, vs)
        assert lines["render"] == rstats and lines["sweep"] == sstats, k
        assert lines["check"] == (0, 0), k
        res = cfg["res"]
        raw = open(dst, "rb").read()
        assert np.array_equal(np.frombuffer(raw[:24 * res * res], dtype=np.float32).reshape(6, res, res), depth), k
        at = 24 * res * res
        assert np.array_equal(np.frombuffer(raw[at:at + len(queries)], dtype=np.uint8), vr.verdict(cfg, depth, c, queries)), k
        cloud = np.frombuffer(raw[at + len(queries):], dtype=np.float64).reshape(-1, 3)
        assert np.array_equal(bucket_sorted(cloud, vs), before[keep]), k
        assert lines["map"] == (len(cloud), len(np.unique(np.floor(cloud / vs), axis=0))), k
        removed_somewhere += sstats[1]
    assert removed_somewhere > 100
