"""2-D LaserScan ingest (kicp_pre_ingest_scan / PreSteps.IngestScan / KinematicICP::IngestScan): the 2-D LiDAR mode of the node
(online_node.cpp:44-58: laser_geometry's projectLaser, then RegisterFrame on the projected cloud).

CPU: the restatement (tests/laserscan_ref.py) against scans worked out by hand, its table cache, a short drive through the okicp
pipeline against the reference's own RegisterFrame, and the drop-in harness compiling against the headers.
GPU: IngestScan against the restatement bit for bit over a grid of sizes, drops, stamps and cutoffs; the table cache; interleaving
with cloud messages on one handle; a 2-D drive through the pre-steps, the registration and the device map update, from Python and
through the drop-in harness.
Recalled details of laser_geometry these tests pin: the float angle a_i = angle_min + (float)i * angle_increment; the table key
(n, angle_min, angle_max) without angle_increment; range_cutoff < 0 -> range_max, a positive cutoff taken as given (also above
range_max); r < cutoff (double) and r >= range_min (float); x, y rounded to float from a double product; stamps
(float)i * time_increment with i the original beam index."""
import math
import subprocess

import numpy as np
import pytest

import laserscan_ref as L
from kinematic_icp_amd import synthetic as syn
from oracle import okicp, rkicp

F32 = np.float32


def hand_point(r, a):
    """x, y of one kept beam, straight from the rules (a: the float32 angle)"""
    return float(F32(float(r) * math.cos(float(a)))), float(F32(float(r) * math.sin(float(a))))


def test_known_answer_scans():
    nan, inf = float("nan"), float("inf")
    ranges = np.array([1.0, nan, 0.5, 10.0, inf, -inf, 3.0, 9.99, 0.4999], dtype=np.float32)
    for inc, tinc in ((0.5, 0.001), (-0.5, -0.001)):
        for cutoff, kept in ((-1.0, [0, 2, 6, 7]), (5.0, [0, 2, 6]), (20.0, [0, 2, 3, 6, 7])):
            p = L.Projector().project(ranges, 0.25, 0.25 + 8 * inc, inc, tinc, 0.5, 10.0, cutoff)
            assert p["n"] == len(kept) and list(p["index"]) == kept
            for row, i in enumerate(kept):
                a = F32(F32(0.25) + F32(F32(i) * F32(inc)))
                assert tuple(p["xyz"][row]) == (*hand_point(ranges[i], a), 0.0)
                assert p["stamps"][row] == F32(F32(i) * F32(tinc))  # the ORIGINAL beam index
            xyz, st, (lo, hi) = L.ingest(p)
            np.testing.assert_array_equal(xyz, p["xyz"])
            s = p["stamps"].astype(np.float64)
            assert (lo, hi) == (s.min(), s.max())
            np.testing.assert_array_equal(st, (s - lo) / (hi - lo))
    # a cutoff exactly on a range drops it; range_min exactly is kept; nothing kept -> no stamps
    p = L.Projector().project(np.array([2.0, 3.0], dtype=np.float32), 0.0, 1.0, 1.0, 0.1, 2.0, 10.0, 3.0)
    assert list(p["index"]) == [0]
    xyz, st, mm = L.ingest(p)
    assert np.isnan(st).all() and mm == (0.0, 0.0)  # one kept beam: (t - min) / (max - min) = 0 / 0, as the reference
    p = L.Projector().project(np.array([nan, inf], dtype=np.float32), 0.0, 1.0, 1.0, 0.1, 2.0, 10.0)
    assert p["n"] == 0 and L.ingest(p)[1] is None
    with np.errstate(invalid="ignore"):
        p = L.Projector().project(np.array([1.0, 2.0], dtype=np.float32), 0.0, 1.0, 1.0, 0.0, 0.5, 10.0)
        assert np.isnan(L.ingest(p)[1]).all()  # time_increment = 0: every stamp equal -> 0 / 0


def test_restatement_table_cache_keeps_angle_increment_out_of_the_key():
    r = np.linspace(1.0, 5.0, 16).astype(np.float32)
    proj = L.Projector()
    a = proj.project(r, -1.0, 1.0, 0.125, 0.0, 0.1, 20.0)
    b = proj.project(r, -1.0, 1.0, 0.25, 0.0, 0.1, 20.0)      # same n / angle_min / angle_max: the stale table
    assert proj.rebuilds == 1
    np.testing.assert_array_equal(a["xyz"], b["xyz"])
    fresh = L.Projector().project(r, -1.0, 1.0, 0.25, 0.0, 0.1, 20.0)
    assert not np.array_equal(fresh["xyz"], b["xyz"])
    c = proj.project(r, -1.0, 2.0, 0.25, 0.0, 0.1, 20.0)       # angle_max changed: rebuilt, now with the new increment
    assert proj.rebuilds == 2
    np.testing.assert_array_equal(c["xyz"], fresh["xyz"])
    proj.project(r[:15], -1.0, 2.0, 0.25, 0.0, 0.1, 20.0)      # n changed
    assert proj.rebuilds == 3


VOXEL, MAX_RANGE, MIN_RANGE = 0.2, 30.0, 0.0


def make_drive(n_frames, zero_tinc_frame=None):
    params, ext, frames = syn.make_laser_drive(n_frames)
    if zero_tinc_frame is not None:
        frames[zero_tinc_frame]["time_increment"] = 0.0
    return params, ext, frames


def restated_clouds(params, frames):
    """per frame: the restatement's projection (one projector for the drive) and okicp.ingest of its packed records"""
    proj, out = L.Projector(), []
    for fr in frames:
        tinc = fr.get("time_increment", params["time_increment"])
        p = proj.project(fr["ranges"], params["angle_min"], params["angle_max"], params["angle_increment"], tinc, params["range_min"],
                         params["range_max"])
        out.append((p, L.ingest(p)))
    return out


class OkicpPipeline:
    """KinematicICP::RegisterFrame re-enacted with the oracle's pieces (pipeline/KinematicICP.cpp:48-85), as tests/test_facade.py"""

    def __init__(self, deskew):
        self.map = okicp.VoxelHashMap(VOXEL, MAX_RANGE, 20)
        self.thr = okicp.CorrespondenceThreshold(VOXEL / np.sqrt(20), MAX_RANGE, True, 1.0)
        self.reg, self.last, self.deskew = okicp.KinematicRegistration(), okicp.IDENTITY.copy(), deskew

    def register(self, xyz, st, ext, dl):
        rel_lidar = okicp.se3_mul(okicp.se3_mul(okicp.se3_inverse(ext), dl), ext)
        pre = okicp.preprocess(xyz, st if st is not None else np.zeros(0), rel_lidar, MAX_RANGE, MIN_RANGE, self.deskew)
        in_base = okicp.se3_act(ext, pre)
        down = okicp.voxel_downsample(in_base, VOXEL * 0.5)
        source = okicp.voxel_downsample(down, VOXEL * 1.5)
        tau = self.thr.ComputeThreshold()
        new = self.reg.ComputeRobotMotion(source, self.map, self.last, dl, tau)
        self.thr.UpdateOdometryError(okicp.se3_mul(okicp.se3_inverse(okicp.se3_mul(self.last, dl)), new))
        self.map.Update(down, new)
        self.last = new
        return new, in_base, source, down, tau


@pytest.mark.parametrize("deskew", [False, True])
def test_restated_drive_through_okicp_equals_the_reference_register_frame(deskew):
    if not rkicp.available():
        pytest.skip("oracle/_ref/libkicp_ref.so missing and /root/reference not present to build it")
    params, ext, frames = make_drive(6, zero_tinc_frame=None if deskew else 3)
    ours = OkicpPipeline(deskew)
    ref = rkicp.KinematicICP(max_range=MAX_RANGE, min_range=MIN_RANGE, voxel_size=VOXEL, deskew=deskew)
    for k, (fr, (p, (xyz, st, _))) in enumerate(zip(frames, restated_clouds(params, frames))):
        pose, in_base, source, _, _ = ours.register(xyz, st, ext, fr["rel_odom"])
        ref_frame, ref_source = ref.RegisterFrame(xyz, st if st is not None else [], ext, fr["rel_odom"])
        np.testing.assert_allclose(pose, ref.pose(), rtol=0, atol=1e-9, err_msg="frame %d" % k)
        assert (len(in_base), len(source)) == (len(ref_frame), len(ref_source)), "frame %d" % k
        assert ours.map.num_points() == len(ref.LocalMap()), "frame %d" % k


def test_laserscan_facade_compiles_and_links():
    """the drop-in's IngestScan (KinematicICP.hpp) and kicp_pre_ingest_scan (kicp.h) exist and link against libkicp_amd.so"""
    assert subprocess.run(["test", "-x", L.build_harness()]).returncode == 0


# ---------------------------------------------------------------------------------------------------------------------------- GPU
def scan_params(n):
    inc = F32(4.71238898 / max(n, 1))
    amin = F32(-2.35619449)
    return dict(angle_min=float(amin), angle_max=float(F32(amin + F32(max(n - 1, 0)) * inc)), angle_increment=float(inc),
                range_min=0.1, range_max=20.0)


def grid_ranges(rng, n, drops):
    f = F32
    r = rng.uniform(0.2, 19.0, n).astype(np.float32)
    bad = np.array([np.nan, np.inf, -np.inf, 0.05, 20.0, 100.0, -1.0], dtype=np.float32)  # 20.0 = range_max: kept only above the cutoff
    if drops == "all":
        r = bad[rng.integers(0, len(bad), n)]
        r[r == f(20.0)] = np.nan
    elif drops == "random":
        m = rng.random(n) < 0.3
        r[m] = bad[rng.integers(0, len(bad), int(m.sum()))]
    elif drops == "boundary":
        edge = np.array([f(0.1), np.nextafter(f(0.1), f(0)), f(20.0), np.nextafter(f(20.0), f(0)), f(15.0), np.nextafter(f(15.0), f(0)),
                         np.nextafter(f(15.0), f(100)), f(25.0), np.nan], dtype=np.float32)
        m = rng.random(n) < 0.5
        r[m] = edge[rng.integers(0, len(edge), int(m.sum()))]
    return r


def assert_ingested_equal(pre, p, xyz, st, mm, got_mm):
    gx, gs = pre.ingested()
    assert gx.shape == xyz.shape
    np.testing.assert_array_equal(gx.view(np.uint64), xyz.view(np.uint64))  # bit for bit (signed zeros included)
    if st is None:
        assert gs is None
    else:
        np.testing.assert_array_equal(gs, st)  # (NaN where the reference divides 0 by 0)
    assert tuple(got_mm) == tuple(mm)


@pytest.mark.gpu
def test_gpu_ingest_scan_equals_the_restatement_bit_for_bit():
    import kinematic_icp_amd as K
    lib = K.lib()
    rng = np.random.Generator(np.random.PCG64(401))
    pre = K.PreSteps()
    cases = 0
    for n in (0, 1, 255, 256, 257, 1080, 4096, 100_003):
        sp = scan_params(n)
        proj = L.Projector()  # one per handle, as the node holds one laser_geometry projector
        for drops in ("none", "all", "random", "boundary"):
            r = grid_ranges(rng, n, drops)
            for tinc in (0.025 / max(n, 1), 0.0, -0.025 / max(n, 1)):
                for cutoff in (-1.0, 15.0, 25.0):
                    p = proj.project(r, sp["angle_min"], sp["angle_max"], sp["angle_increment"], tinc, sp["range_min"], sp["range_max"], cutoff)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        xyz, st, mm = L.ingest(p)
                    got = pre.IngestScan(r, sp["angle_min"], sp["angle_max"], sp["angle_increment"], tinc, sp["range_min"], sp["range_max"], cutoff)
                    what = "n %d drops %s tinc %r cutoff %r" % (n, drops, tinc, cutoff)
                    assert lib.kicp_pre_ingested_count(pre._h) == p["n"], what
                    assert_ingested_equal(pre, p, xyz, st, mm, got)
                    # ... and what Ingest makes of the restatement's packed records, on the same handle
                    got_cloud = pre.Ingest(p["packed"], p["n"], *L.LAYOUT)
                    assert_ingested_equal(pre, p, xyz, st, mm, got_cloud)
                    cases += 1
        assert proj.rebuilds == 1
    assert cases == 8 * 4 * 3 * 3


@pytest.mark.gpu
def test_gpu_ingest_scan_table_cache():
    import kinematic_icp_amd as K
    pre, proj = K.PreSteps(), L.Projector()
    rng = np.random.Generator(np.random.PCG64(402))
    r = rng.uniform(0.5, 10.0, 1080).astype(np.float32)
    sp = scan_params(1080)
    args = lambda inc, amax: (sp["angle_min"], amax, inc, 1e-5, 0.1, 20.0)  # noqa: E731
    inc2 = float(F32(sp["angle_increment"] * 0.5))
    for a in (args(sp["angle_increment"], sp["angle_max"]), args(inc2, sp["angle_max"]), args(inc2, sp["angle_max"] + 0.5)):
        p = proj.project(r, *a)
        mm = pre.IngestScan(r, *a)
        xyz, st, omm = L.ingest(p)
        assert_ingested_equal(pre, p, xyz, st, omm, mm)
        if a[2] == inc2 and a[1] == sp["angle_max"]:  # the stale table was used: a fresh projector would give other points
            assert not np.array_equal(L.Projector().project(r, *a)["xyz"], xyz)
    assert proj.rebuilds == 2


def packed_cloud(rng, n):
    rec = np.zeros((n, 4), dtype=np.float32)
    rec[:, :3] = rng.uniform(-20.0, 20.0, (n, 3))
    rec[:, 2] *= 0.1
    rec[:, 3] = np.linspace(0.0, 0.1, n)
    return rec.tobytes()


@pytest.mark.gpu
def test_gpu_scans_and_clouds_interleave_on_one_handle():
    import kinematic_icp_amd as K
    rng = np.random.Generator(np.random.PCG64(403))
    pre = K.PreSteps()
    params, ext, frames = make_drive(4)
    restated = restated_clouds(params, frames)
    cloud = np.frombuffer(packed_cloud(rng, 5000), dtype=np.uint8).copy()
    cxyz, cst, cmm = okicp.ingest(cloud, 5000, *L.LAYOUT)
    sargs = lambda k: (frames[k]["ranges"], params["angle_min"], params["angle_max"], params["angle_increment"], params["time_increment"],  # noqa: E731
                       params["range_min"], params["range_max"])
    # an announced cloud, then a scan: the scan is right and the announcement void
    pre.IngestAhead(cloud, 5000, *L.LAYOUT)
    hits = pre.ahead_hits()
    p, (xyz, st, mm) = restated[0]
    assert_ingested_equal(pre, p, xyz, st, mm, pre.IngestScan(*sargs(0)))
    assert_ingested_equal(pre, None, cxyz, cst, cmm, pre.Ingest(cloud, 5000, *L.LAYOUT))
    assert pre.ahead_hits() == hits
    # scan and cloud frames alternate through the chained pre-steps
    rel = syn.planar_pose(0.2, 0.0, np.deg2rad(2.0))
    rel_lidar = okicp.se3_mul(okicp.se3_mul(okicp.se3_inverse(ext), rel), ext)
    for k in range(4):
        for kind in ("scan", "cloud"):
            if kind == "scan":
                pre.IngestScan(*sargs(k))
                _, (xyz, st, _) = restated[k]
            else:
                pre.Ingest(cloud, 5000, *L.LAYOUT)
                xyz, st = cxyz, cst
            counts, out = pre.Frame(None, None, rel_lidar, ext, MAX_RANGE, MIN_RANGE, False, VOXEL * 0.5, VOXEL * 1.5)
            in_base = okicp.se3_act(ext, okicp.preprocess(xyz, st, rel_lidar, MAX_RANGE, MIN_RANGE, False))
            down = okicp.voxel_downsample(in_base, VOXEL * 0.5)
            assert counts == [len(in_base), len(down), len(okicp.voxel_downsample(down, VOXEL * 1.5))], (k, kind)
            np.testing.assert_allclose(out, in_base, rtol=0, atol=1e-11, err_msg="%d %s" % (k, kind))


@pytest.mark.gpu
@pytest.mark.parametrize("deskew", [False, True])
def test_gpu_laser_drive_through_the_pipeline(deskew):
    """IngestScan -> Frame(None, ...) -> registration -> device map update over a 24-frame drive, against the okicp composition
    and the reference's RegisterFrame.  Deskew off: one frame has time_increment = 0.  Deskew on: such a frame's stamps are pinned
    at the ingest (all NaN, the reference's 0 / 0) and kept out of the drive."""
    import kinematic_icp_amd as K
    params, ext, frames = make_drive(24, zero_tinc_frame=None if deskew else 11)
    restated = restated_clouds(params, frames)
    pre, reg = K.PreSteps(), K.KinematicRegistration(device=0)
    gmap = K.VoxelHashMap(VOXEL, MAX_RANGE, 20)
    ours = OkicpPipeline(deskew)
    ref = rkicp.KinematicICP(max_range=MAX_RANGE, min_range=MIN_RANGE, voxel_size=VOXEL, deskew=deskew) if rkicp.available() else None
    last, on_device = okicp.IDENTITY.copy(), 0
    for k, (fr, (p, (xyz, st, mm))) in enumerate(zip(frames, restated)):
        tinc = fr.get("time_increment", params["time_increment"])
        got = pre.IngestScan(fr["ranges"], params["angle_min"], params["angle_max"], params["angle_increment"], tinc, params["range_min"],
                             params["range_max"])
        assert_ingested_equal(pre, p, xyz, st, mm, got)
        dl = fr["rel_odom"]
        rel_lidar = okicp.se3_mul(okicp.se3_mul(okicp.se3_inverse(ext), dl), ext)
        counts, out = pre.Frame(None, None, rel_lidar, ext, MAX_RANGE, MIN_RANGE, deskew, VOXEL * 0.5, VOXEL * 1.5)
        new, in_base, source, down, tau = ours.register(xyz, st, ext, dl)
        assert counts == [len(in_base), len(down), len(source)], "frame %d" % k
        np.testing.assert_allclose(out, in_base, rtol=0, atol=1e-11, err_msg="frame %d" % k)
        pose = reg.ComputeRobotMotion(pre.frame(2), gmap, last, dl, tau)
        np.testing.assert_allclose(pose, new, rtol=0, atol=1e-12, err_msg="frame %d" % k)
        on_device += int(gmap.UpdateDevice(pre.frame(1), pose))
        assert gmap.num_points() == ours.map.num_points(), "frame %d" % k
        last = pose
        if ref is not None:
            ref_frame, ref_source = ref.RegisterFrame(xyz, st if st is not None else [], ext, dl)
            np.testing.assert_allclose(pose, ref.pose(), rtol=0, atol=1e-9, err_msg="frame %d vs reference build" % k)
            assert (len(ref_frame), len(ref_source)) == (counts[0], counts[2]), "frame %d vs reference build" % k
    assert on_device > 0
    if deskew:  # time_increment = 0 with deskew on: every kept stamp equal -> NaN after normalisation, at the ingest
        r = frames[0]["ranges"]
        mm = pre.IngestScan(r, params["angle_min"], params["angle_max"], params["angle_increment"], 0.0, params["range_min"], params["range_max"])
        assert mm == (0.0, 0.0) and pre.ingested()[1] is not None and np.isnan(pre.ingested()[1]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("deskew", [False, True])
def test_gpu_laser_drive_through_the_drop_in(tmp_path, deskew):
    """the same drive through KinematicICP::IngestScan + RegisterIngestedFrame (tests/cpp/laserscan_facade_test)"""
    params, ext, frames = make_drive(24, zero_tinc_frame=None if deskew else 11)
    f = tmp_path / "scan.bin"
    L.write_drive(f, params, ext, frames, VOXEL, MAX_RANGE, MIN_RANGE, deskew)
    out = subprocess.check_output([L.build_harness(), "scan_pipeline", str(f)], text=True).splitlines()
    assert len(out) == 3 * len(frames)
    ours = OkicpPipeline(deskew)
    ref = rkicp.KinematicICP(max_range=MAX_RANGE, min_range=MIN_RANGE, voxel_size=VOXEL, deskew=deskew) if rkicp.available() else None
    for k, (fr, (p, (xyz, st, mm))) in enumerate(zip(frames, restated_clouds(params, frames))):
        pose = np.array([float(x) for x in out[3 * k].split()[1:]])
        sizes = [int(x) for x in out[3 * k + 1].split()[1:]]
        stamps = out[3 * k + 2].split()
        assert stamps[1] == ("1" if p["n"] else "0") and (float(stamps[2]), float(stamps[3])) == mm, "frame %d" % k
        new, in_base, source, _, _ = ours.register(xyz, st, ext, fr["rel_odom"])
        np.testing.assert_allclose(pose, new, rtol=0, atol=1e-12, err_msg="frame %d" % k)
        assert sizes == [len(in_base), len(source), ours.map.num_points()], "frame %d" % k
        if ref is not None:
            ref.RegisterFrame(xyz, st if st is not None else [], ext, fr["rel_odom"])
            np.testing.assert_allclose(pose, ref.pose(), rtol=0, atol=1e-9, err_msg="frame %d vs reference build" % k)
