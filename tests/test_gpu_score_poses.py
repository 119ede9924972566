"""kicp_score_poses: DataAssociation (registration/Registration.cpp:62-81) of ONE frame at many poses in one call.  Per pose the
number of correspondences and the sum of their squared residuals must be THE SAME DOUBLES kicp_pass_sums returns at that pose
(sums[6] and sums[5]) - for every frame size around the 64-lane wave and the 256-point tile, for one pose and for hundreds, however
the (pose x point) space is cut into launches ("score_chunk"), at tight and loose thresholds, on the tie scenes of tests/tie_cases.py,
wherever the map's newest state lives - and must agree with the CPU oracle's pass to the tolerances tests/test_gpu_parity.py holds
kicp_pass_sums itself to."""
import ctypes as C

import numpy as np
import pytest

import kinematic_icp_amd as K
from kinematic_icp_amd import synthetic as syn
from checkers import okicp
import tie_cases as tc

pytestmark = pytest.mark.gpu

SUM_RTOL, SUM_ATOL = 1e-10, 1e-9  # tests/test_gpu_parity.py:18,82 - the same quantities against the same oracle
SIZES = [1, 63, 64, 65, 255, 256, 257, 854]
COUNTS = [1, 2, 7, 64, 300]
IDENT = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def _keypoints(cfg, frame):
    """the registration source of the pipeline: two voxel downsamples (pipeline/KinematicICP.cpp:61-62)"""
    return okicp.voxel_downsample(okicp.voxel_downsample(frame, cfg.voxel_size * 0.5), cfg.voxel_size * 1.5)


def _poses(scan, rng, count):
    """the guess, the truth, a pose 500 m away (no correspondence at all), an exact duplicate of the guess, then planar offsets of the
    guess up to 2 m / 20 degrees"""
    guess = syn.pose_mul(scan["last_pose"], scan["rel_odom"])
    poses = [guess, scan["true_pose"], syn.pose_mul(guess, syn.planar_pose(500.0, 0.0, 0.3)), guess.copy()]
    while len(poses) < count:
        poses.append(syn.pose_mul(guess, syn.planar_pose(rng.uniform(-2, 2), rng.uniform(-2, 2), np.deg2rad(rng.uniform(-20, 20)))))
    return np.array(poses[:count])


def _generic():
    reg = K.KinematicRegistration()
    reg.set_option("small", 0)
    return reg


def _pass_sums(reg, frame, gmap, poses, tau):
    """(n_corr, ssr) pose by pose from kicp_pass_sums: the reference every test below compares with"""
    sums = np.array([reg.pass_sums(frame, gmap, p, tau) for p in poses]).reshape(-1, 7)
    return sums[:, 6], sums[:, 5]


@pytest.fixture(scope="module")
def case1():
    cfg, scene, scans, rng = syn.make_case("cfg1", n_scans=2)
    gmap = K.VoxelHashMap(cfg.voxel_size, cfg.max_range, cfg.max_points_per_voxel)
    syn.build_map_points(scene, cfg, gmap.AddPoints, gmap.num_points, rng)
    omap = okicp.VoxelHashMap(cfg.voxel_size, cfg.max_range, cfg.max_points_per_voxel)
    omap.AddPoints(gmap.Pointcloud())
    keypoints = _keypoints(cfg, scans[0]["frame"])
    assert 700 <= len(keypoints) <= 1000  # (about 850; SIZES' last entry stands for "all of them")
    poses = _poses(scans[0], np.random.default_rng(11), max(COUNTS))
    return cfg, scans, gmap, omap, keypoints, poses


@pytest.fixture(scope="module")
def handles():
    return K.KinematicRegistration(), _generic()


@pytest.fixture(scope="module")
def references(case1, handles):
    """kicp_pass_sums at every pose for every frame size, once, on both handles (computed on first use per size)"""
    cfg, scans, gmap, omap, keypoints, poses = case1
    cache = {}

    def get(n):
        if n not in cache:
            frame = keypoints[:min(n, len(keypoints))]
            cache[n] = [_pass_sums(reg, frame, gmap, poses, cfg.first_frame_tau()) for reg in handles]
        return cache[n]
    return get


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_scores_are_pass_sums_bit_for_bit(case1, handles, references, n, count):
    cfg, scans, gmap, omap, keypoints, poses = case1
    frame = keypoints[:min(n, len(keypoints))]
    for reg, (want_n, want_ssr) in zip(handles, references(n)):
        n_corr, ssr = reg.ScorePoses(frame, gmap, poses[:count], cfg.first_frame_tau())
        assert np.array_equal(n_corr, want_n[:count])
        assert np.array_equal(ssr, want_ssr[:count])
        assert reg.get_option("score_launches") == 1
    if count >= 7:
        assert n_corr[2] == 0 and ssr[2] == 0            # 500 m away: a result, not a warning
        assert (n_corr[3], ssr[3]) == (n_corr[0], ssr[0])  # the duplicate
    if n >= 255:
        assert n_corr[0] > 0.5 * len(frame) and ssr[0] > 0


def test_scores_match_the_oracle(case1, handles):
    cfg, scans, gmap, omap, keypoints, poses = case1
    tau = cfg.first_frame_tau()
    n_corr, ssr = handles[0].ScorePoses(keypoints, gmap, poses[:64], tau)
    for k in range(64):
        o, _ = okicp.icp_pass(omap, keypoints, poses[k], tau)
        assert n_corr[k] == o[6]
        np.testing.assert_allclose(ssr[k], o[5], rtol=SUM_RTOL, atol=SUM_ATOL)
    assert n_corr.max() > 0.9 * len(keypoints) and (n_corr < 0.5 * len(keypoints)).any()  # good and bad hypotheses both present


@pytest.mark.parametrize("chunk,at_least", [(1024, 3), (100, 14)], ids=["four_tiles_per_launch", "less_than_one_pose"])
def test_splitting_into_launches_changes_nothing(case1, chunk, at_least):
    """n = 257 (two tiles), count = 7: 14 (tile, pose) items; a launch serves floor(chunk / 256) of them, at least one"""
    cfg, scans, gmap, omap, keypoints, poses = case1
    reg = K.KinematicRegistration()
    whole = reg.ScorePoses(keypoints[:257], gmap, poses[:7], cfg.first_frame_tau())
    assert reg.get_option("score_launches") == 1
    reg.set_option("score_chunk", chunk)
    assert reg.get_option("score_chunk") == chunk
    split = reg.ScorePoses(keypoints[:257], gmap, poses[:7], cfg.first_frame_tau())
    assert reg.get_option("score_launches") >= at_least
    assert np.array_equal(split[0], whole[0]) and np.array_equal(split[1], whole[1])
    assert whole[0][0] > 100


@pytest.mark.parametrize("scale", [0.25, 1.0, 3.0])
def test_thresholds(case1, handles, scale):
    cfg, scans, gmap, omap, keypoints, poses = case1
    tau = scale * cfg.first_frame_tau()
    for reg in handles:
        n_corr, ssr = reg.ScorePoses(keypoints, gmap, poses[:7], tau)
        want_n, want_ssr = _pass_sums(reg, keypoints, gmap, poses[:7], tau)
        assert np.array_equal(n_corr, want_n) and np.array_equal(ssr, want_ssr)
    assert n_corr[0] > 0


@pytest.mark.parametrize("copies", [1, 60])
def test_tie_scenes(handles, copies):
    """tests/tie_cases.py: equidistant candidates, candidates an ulp apart with equal norms, candidates the mirror orders the other way
    round, candidates exactly at tau - a wrong pick moves a residual by >= 0.3 m, i.e. the sum by far more than its last bit"""
    scene = tc.build(copies)
    gmap = K.VoxelHashMap(tc.VS, 100.0, tc.CAP)
    gmap.AddPoints(scene.map_points)
    poses = np.array([IDENT, IDENT])
    want = ~np.isnan(scene.expected[:, 0])
    for reg in handles:
        n_corr, ssr = reg.ScorePoses(scene.queries, gmap, poses, tc.TAU)
        want_n, want_ssr = _pass_sums(reg, scene.queries, gmap, poses, tc.TAU)
        assert np.array_equal(n_corr, want_n) and np.array_equal(ssr, want_ssr)
        assert n_corr[0] == want.sum()


def test_map_placement_empty_map_and_nan_pose(case1, handles):
    cfg, scans, gmap, omap, keypoints, poses = case1
    tau = cfg.first_frame_tau()
    reg = handles[0]
    dmap = K.VoxelHashMap(cfg.voxel_size, cfg.max_range, cfg.max_points_per_voxel)
    cloud = gmap.Pointcloud()
    assert dmap.UpdateDevice(K.DeviceFrame(cloud), IDENT)  # device-authoritative: the newest state lives in HBM only
    for placed in ("device", "host"):
        if placed == "host":
            dmap.Clear(), dmap.AddPoints(cloud)
        n_corr, ssr = reg.ScorePoses(keypoints, dmap, poses[:7], tau)
        want_n, want_ssr = _pass_sums(reg, keypoints, dmap, poses[:7], tau)
        assert np.array_equal(n_corr, want_n) and np.array_equal(ssr, want_ssr)
        assert n_corr[0] > 0.5 * len(keypoints)
    # an update begun and not yet collected is collected by the call (the frame stays alive until then)
    pending = K.DeviceFrame(keypoints)
    dmap.UpdateDevice(K.DeviceFrame(cloud), IDENT)
    dmap.UpdateDeviceBegin(pending, poses[1])
    n_corr, ssr = reg.ScorePoses(keypoints, dmap, poses[:2], tau)
    want_n, want_ssr = _pass_sums(reg, keypoints, dmap, poses[:2], tau)
    assert np.array_equal(n_corr, want_n) and np.array_equal(ssr, want_ssr)
    # an empty map, an empty frame, no poses: zeros, no launch
    empty = K.VoxelHashMap(1.0, 100.0, 20)
    n_corr, ssr = reg.ScorePoses(keypoints, empty, poses[:7], tau)
    assert not n_corr.any() and not ssr.any() and reg.get_option("score_launches") == 0
    n_corr, ssr = reg.ScorePoses(np.zeros((0, 3)), gmap, poses[:7], tau)
    assert n_corr.shape == (7,) and not n_corr.any() and not ssr.any()
    n_corr, ssr = reg.ScorePoses(keypoints, gmap, np.zeros((0, 7)), tau)
    assert n_corr.shape == (0,) and ssr.shape == (0,)
    # a NaN pose gives what kicp_pass_sums gives, and does not disturb its neighbours
    with_nan = np.array([poses[0], np.full(7, np.nan), poses[1]])
    n_corr, ssr = reg.ScorePoses(keypoints, gmap, with_nan, tau)
    want_n, want_ssr = _pass_sums(reg, keypoints, gmap, with_nan, tau)
    assert np.array_equal(n_corr, want_n, equal_nan=True) and np.array_equal(ssr, want_ssr, equal_nan=True)
    assert n_corr[0] > 0 and n_corr[2] > 0


def test_device_frame_equals_host_frame(case1, handles):
    cfg, scans, gmap, omap, keypoints, poses = case1
    for reg in handles:
        host = reg.ScorePoses(keypoints, gmap, poses[:64], cfg.first_frame_tau())
        dev = reg.ScorePoses(K.DeviceFrame(keypoints), gmap, poses[:64], cfg.first_frame_tau())
        assert np.array_equal(host[0], dev[0]) and np.array_equal(host[1], dev[1])


def test_full_size_scan_on_cfg2():
    """BASELINE.json configs[1]: the 131 072-point scan (512 tiles) against the ~1M-point map, four poses"""
    cfg, scene, scans, rng = syn.make_case("cfg2", n_scans=1)
    gmap = K.VoxelHashMap(cfg.voxel_size, cfg.max_range, cfg.max_points_per_voxel)
    syn.build_map_points(scene, cfg, lambda pts: gmap.UpdateDevice(K.DeviceFrame(pts), IDENT), gmap.num_points, rng)
    s = scans[0]
    guess = syn.pose_mul(s["last_pose"], s["rel_odom"])
    poses = np.array([guess, s["true_pose"], syn.pose_mul(guess, syn.planar_pose(0.7, -0.4, np.deg2rad(5.0))), syn.pose_mul(guess, syn.planar_pose(500.0, 0.0, 0.0))])
    reg = K.KinematicRegistration()
    n_corr, ssr = reg.ScorePoses(s["frame"], gmap, poses, cfg.first_frame_tau())
    want_n, want_ssr = _pass_sums(reg, s["frame"], gmap, poses, cfg.first_frame_tau())
    assert np.array_equal(n_corr, want_n) and np.array_equal(ssr, want_ssr)
    assert len(s["frame"]) == 131072 and n_corr[0] > 0.5 * 131072 and n_corr[3] == 0


def test_errors(case1):
    cfg, scans, gmap, omap, keypoints, poses = case1
    tau = cfg.first_frame_tau()
    reg = K.KinematicRegistration()
    lib = K.lib()
    dp = C.POINTER(C.c_double)
    frame = np.ascontiguousarray(keypoints[:64])
    q = np.ascontiguousarray(poses[:2])
    out_n, out_s = np.zeros(2), np.zeros(2)
    fp, qp, np_, sp = (a.ctypes.data_as(dp) for a in (frame, q, out_n, out_s))
    # null pointers
    for args in ((None, gmap._h, fp, 64, qp, 2, tau, np_, sp), (reg._h, None, fp, 64, qp, 2, tau, np_, sp), (reg._h, gmap._h, None, 64, qp, 2, tau, np_, sp),
                 (reg._h, gmap._h, fp, 64, None, 2, tau, np_, sp), (reg._h, gmap._h, fp, 64, qp, 2, tau, None, sp), (reg._h, gmap._h, fp, 64, qp, 2, tau, np_, None)):
        assert lib.kicp_score_poses(*args) == K.KICP_ERR_ARG
        assert b"null argument" in lib.kicp_last_error()
    # documented limits (checked before anything is read: the arrays need not be that long)
    assert lib.kicp_score_poses(reg._h, gmap._h, fp, 64, qp, (1 << 24) + 1, tau, np_, sp) == K.KICP_ERR_CAPACITY
    assert lib.kicp_score_poses(reg._h, gmap._h, fp, 0x7FFFFFF0 // 3 + 1, qp, 2, tau, np_, sp) == K.KICP_ERR_CAPACITY
    assert lib.kicp_score_poses_device(reg._h, gmap._h, None, 64, qp, 2, tau, np_, sp) == K.KICP_ERR_ARG
    # a multi-GPU exchange attached to the handle: scored per device only, in kicp_pass_correspondences' words
    sharded = K.KinematicRegistration()
    sharded.set_allreduce(lambda ptr, count, stream: None)
    with pytest.raises(K.KicpError) as e:
        sharded.ScorePoses(keypoints, gmap, poses[:2], tau)
    assert e.value.code == K.KICP_ERR_ARG and "detach the multi-GPU exchange first" in str(e.value)
    with pytest.raises(K.KicpError) as e:
        sharded.pass_correspondences(keypoints, gmap, poses[0], tau)
    assert "detach the multi-GPU exchange first" in str(e.value)
    # the handle is as good as before
    n_corr, ssr = reg.ScorePoses(keypoints, gmap, poses[:2], tau)
    assert n_corr[0] > 0
