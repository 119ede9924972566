"""kicp_planar_sums / kicp_refine_poses_planar / kicp_relocalize_planar on the GPU.

Sums: N, S_y, S_ss, S_a, S_c and ssr must be THE SAME DOUBLES kicp_pass_sums returns at that pose (elements [6], -[1], [2], [3], [4],
[5]: the pass kernels' own terms) - for every frame size around the 64-lane wave and the 256-point tile, for one pose and for hundreds,
however the (pose x point) space is cut into launches, on the tie scenes, wherever the map's newest state lives.  S_x and S_b, the two
sums a pass does not form, are held against tests/planar_ref.py fed with kicp_pass_correspondences at the same pose, to tolerances
derived from the arithmetic (see the test).
Refinement: bit-equal to a Python loop of {PlanarSums of ONE pose, planar_step}; RelocalizePlanar bit-equal to its restatement from
ScorePoses + RefinePosesPlanar + ScorePoses + arg-min.  Recovery: the case tests/test_planar_host.py pins on the oracle alone."""
import ctypes as C

import numpy as np
import pytest

import kinematic_icp_amd as K
from kinematic_icp_amd import synthetic as syn
from checkers import okicp
import planar_ref as pr
import tie_cases as tc
from test_planar_host import TOP_M, cost_of, offset, recovery_case

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 854]
COUNTS = [1, 2, 7, 64, 300]
IDENT = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
EPS = np.finfo(np.float64).eps


def _keypoints(cfg, frame):
    return okicp.voxel_downsample(okicp.voxel_downsample(frame, cfg.voxel_size * 0.5), cfg.voxel_size * 1.5)


def _poses(scan, rng, count):
    """the pose set of tests/test_gpu_score_poses.py: the guess, the truth, a pose 500 m away, an exact duplicate of the guess, then
    planar offsets of the guess up to 2 m / 20 degrees"""
    guess = syn.pose_mul(scan["last_pose"], scan["rel_odom"])
    poses = [guess, scan["true_pose"], syn.pose_mul(guess, syn.planar_pose(500.0, 0.0, 0.3)), guess.copy()]
    while len(poses) < count:
        poses.append(syn.pose_mul(guess, syn.planar_pose(rng.uniform(-2, 2), rng.uniform(-2, 2), np.deg2rad(rng.uniform(-20, 20)))))
    return np.array(poses[:count])


def _pass_sums(reg, frame, gmap, poses, tau):
    return np.array([reg.pass_sums(frame, gmap, p, tau) for p in poses]).reshape(-1, 7)


def _assert_shared_sums(sums, want):
    """the six sums whose terms are the pass kernels' own: the same doubles"""
    assert np.array_equal(sums[:, 0], want[:, 6], equal_nan=True)
    assert np.array_equal(sums[:, 7], want[:, 5], equal_nan=True)
    assert np.array_equal(sums[:, 2], -want[:, 1], equal_nan=True)
    assert np.array_equal(sums[:, 3], want[:, 2], equal_nan=True)
    assert np.array_equal(sums[:, 4], want[:, 3], equal_nan=True)
    assert np.array_equal(sums[:, 6], want[:, 4], equal_nan=True)


@pytest.fixture(scope="module")
def case1():
    cfg, scene, scans, rng = syn.make_case("cfg1", n_scans=2)
    gmap = K.VoxelHashMap(cfg.voxel_size, cfg.max_range, cfg.max_points_per_voxel)
    syn.build_map_points(scene, cfg, gmap.AddPoints, gmap.num_points, rng)
    keypoints = _keypoints(cfg, scans[0]["frame"])
    assert 700 <= len(keypoints) <= 1000  # (about 850; SIZES' last entry stands for "all of them")
    poses = _poses(scans[0], np.random.default_rng(11), max(COUNTS))
    return cfg, scans, gmap, keypoints, poses


@pytest.fixture(scope="module")
def handles():
    generic = K.KinematicRegistration()
    generic.set_option("small", 0)
    return K.KinematicRegistration(), generic


@pytest.fixture(scope="module")
def references(case1, handles):
    """kicp_pass_sums at every pose for every frame size, once, on both handles (computed on first use per size)"""
    cfg, scans, gmap, keypoints, poses = case1
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = [_pass_sums(reg, keypoints[:min(n, len(keypoints))], gmap, poses, cfg.first_frame_tau()) for reg in handles]
        return cache[n]
    return get


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_shared_sums_are_pass_sums_bit_for_bit(case1, handles, references, n, count):
    cfg, scans, gmap, keypoints, poses = case1
    frame = keypoints[:min(n, len(keypoints))]
    for reg, want in zip(handles, references(n)):
        sums = reg.PlanarSums(frame, gmap, poses[:count], cfg.first_frame_tau())
        assert sums.shape == (count, 8)
        _assert_shared_sums(sums, want[:count])
        assert reg.get_option("score_launches") == 1
    if count >= 7:
        assert not sums[2].any()                 # 500 m away: a zero row
        assert np.array_equal(sums[3], sums[0])  # the duplicate
    if n >= 255:
        assert sums[0, 0] > 0.5 * len(frame) and sums[0, 7] > 0


@pytest.mark.parametrize("n", [65, 257, 854])
def test_the_two_new_sums(case1, handles, n):
    """S_x and S_b against planar_ref on the correspondences kicp_pass_correspondences reports at the same pose (math.fsum: the reference's
    own error is half an ulp).  S_x: the source coordinates are exact, every term is rounded once to 2^-40 (to_fixed, |error| <= 2^-41)
    and added exactly.  S_b: b = c1 . r with |r| < tau - the reference forms T s and c1 by the library's own operations (planar_ref.rotate),
    so r is the same double; what differs is the three-term dot product (fused in the kernel, plain in numpy: a few eps tau per term,
    bounded by 16 eps tau with the basis' own rounding) and again the 2^-41 of to_fixed."""
    cfg, scans, gmap, keypoints, poses = case1
    tau = cfg.first_frame_tau()
    frame = keypoints[:min(n, len(keypoints))]
    for reg in handles:
        sums = reg.PlanarSums(frame, gmap, poses[:7], tau)
        for k in range(7):
            idx, d2, nn = reg.pass_correspondences(frame, gmap, poses[k], tau)
            ref = pr.planar_sums_from(idx >= 0, nn, frame, poses[k])
            count = ref[0]
            assert sums[k, 0] == count
            err_x, err_b = abs(sums[k, 1] - ref[1]), abs(sums[k, 5] - ref[5])
            print("n %d pose %d: N %d, |S_x - ref| %.3e (bound %.3e), |S_b - ref| %.3e (bound %.3e)" %
                  (n, k, count, err_x, count * 2.0 ** -41 + np.spacing(abs(ref[1])), err_b, count * (2.0 ** -41 + 16 * EPS * tau)))
            assert err_x <= count * 2.0 ** -41 + np.spacing(abs(ref[1]))
            assert err_b <= count * (2.0 ** -41 + 16 * EPS * tau)
    assert sums[0, 0] > 0.5 * len(frame)


@pytest.mark.parametrize("chunk,at_least", [(1024, 3), (100, 14)], ids=["four_tiles_per_launch", "less_than_one_pose"])
def test_splitting_into_launches_changes_nothing(case1, chunk, at_least):
    """n = 257 (two tiles), count = 7: 14 (tile, pose) items; a launch serves floor(chunk / 256) of them, at least one"""
    cfg, scans, gmap, keypoints, poses = case1
    reg = K.KinematicRegistration()
    whole = reg.PlanarSums(keypoints[:257], gmap, poses[:7], cfg.first_frame_tau())
    assert reg.get_option("score_launches") == 1
    reg.set_option("score_chunk", chunk)
    split = reg.PlanarSums(keypoints[:257], gmap, poses[:7], cfg.first_frame_tau())
    assert reg.get_option("score_launches") >= at_least
    assert np.array_equal(split, whole)
    assert whole[0, 0] > 100


def _refine_set(scans, poses, count):
    """poses[:count] with, from seven poses on, a NaN pose, a pose 1 cm and a pose 0.5 m from the truth among them"""
    start = poses[:count].copy()
    if count >= 7:
        start[4] = np.nan
        start[5] = syn.pose_mul(scans[0]["true_pose"], syn.planar_pose(0.01, 0.0, 0.0))
        start[6] = syn.pose_mul(scans[0]["true_pose"], syn.planar_pose(0.5, 0.0, 0.0))
    return start


def _refine_restated(reg, frame, gmap, start, tau, max_iterations, convergence):
    """the loop of kicp_refine_poses_planar pose by pose: PlanarSums of ONE pose, planar_step"""
    out, iterations, status = start.copy(), np.zeros(len(start), dtype=np.int32), np.full(len(start), 2, dtype=np.int32)
    for k in range(len(start)):
        while True:
            step = K.planar_step(reg.PlanarSums(frame, gmap, out[k:k + 1], tau)[0], out[k])
            if step is None:
                break
            out[k] = step[0]
            iterations[k] += 1
            if np.sqrt(step[1][0] * step[1][0] + step[1][1] * step[1][1] + step[1][2] * step[1][2]) < convergence:
                status[k] = 0
                break
            if iterations[k] >= max_iterations:
                status[k] = 1
                break
    return out, iterations, status


@pytest.mark.parametrize("n,count,max_iterations", [(64, 7, 5), (257, 64, 5), (854, 7, 100), (1, 2, 3)])
def test_refinement_equals_its_restatement(case1, n, count, max_iterations):
    cfg, scans, gmap, keypoints, poses = case1
    tau = cfg.first_frame_tau()
    frame = keypoints[:min(n, len(keypoints))]
    start = _refine_set(scans, poses, count)
    reg = K.KinematicRegistration()
    want = _refine_restated(reg, frame, gmap, start, tau, max_iterations, 1e-4)
    for source in (frame, K.DeviceFrame(frame)):
        got = reg.RefinePosesPlanar(source, gmap, start, tau, max_iterations, 1e-4)
        launches = reg.get_option("score_launches")
        for g, w in zip(got, want):
            assert np.array_equal(g, w, equal_nan=True)
        assert launches == (got[1] + (got[2] == 2)).max()  # one launch per lock-step iteration; a degenerate step took a launch to find out
    out, iterations, status = got
    if n == 1:
        assert (status == 2).all() and not iterations.any() and np.array_equal(out, start)  # one point: no step
        return
    assert status[2] == 2 and iterations[2] == 0 and np.array_equal(out[2], start[2])  # 500 m away
    assert status[4] == 2 and iterations[4] == 0 and np.isnan(out[4]).all()           # the NaN pose
    if max_iterations == 5 and n == 257:
        assert status[6] == 1 and iterations[6] == 5  # 0.5 m away: five steps are not enough
    if max_iterations == 100:
        assert status[5] == 0 and 1 <= iterations[5] < 100  # 1 cm away


def _relocalize_restated(reg, keypoints, gmap, grid, tau, top_m, refine):
    """kicp_relocalize / kicp_relocalize_planar from ScorePoses + a refinement + ScorePoses + arg-min;
    refine(finalists' poses) -> (poses, out of the running)"""
    n = len(keypoints)
    n_corr, ssr = reg.ScorePoses(keypoints, gmap, grid, tau)
    cost = cost_of(n, n_corr, ssr, tau)
    finalists = np.argsort(cost, kind="stable")[:min(top_m, len(grid))]
    refined, out = refine(grid[finalists])
    n_after, ssr_after = reg.ScorePoses(keypoints, gmap, refined, tau)
    best = None
    for j in range(len(finalists)):
        if out[j]:
            continue
        c = cost_of(n, n_after[j], ssr_after[j], tau)
        if best is None or c < best[0]:
            best = (c, int(finalists[j]), refined[j])
    return best[2], best[1], cost[best[1]], best[0]


@pytest.fixture(scope="module")
def recovery_gpu():
    cfg, omap, items = recovery_case()
    gmap = K.VoxelHashMap(cfg.voxel_size, cfg.max_range, cfg.max_points_per_voxel)
    gmap.AddPoints(omap.Pointcloud())  # (every voxel's points in their order: tests/checkers.py ref_map_like)
    assert gmap.num_points() == omap.num_points()
    return cfg, gmap, items


@pytest.mark.parametrize("top_m", [1, 3, 8, 1000])
def test_relocalize_planar_equals_its_restatement(recovery_gpu, top_m):
    cfg, gmap, items = recovery_gpu
    keypoints, truth, _ = items[0]
    tau = cfg.first_frame_tau()
    center = syn.pose_mul(truth, syn.planar_pose(2.8 * 0.25, -1.6 * 0.25, 2.7 * np.deg2rad(3.0)))  # the grid of tests/test_gpu_relocalize.py
    grid = K.planar_grid(center, 0.5, 0.5, np.deg2rad(3.0), 0.25, 0.25, np.deg2rad(3.0))
    assert grid.shape == (75, 7)
    reg = K.KinematicRegistration()

    def planar(start):
        poses, iterations, status = reg.RefinePosesPlanar(keypoints, gmap, start, tau, 100, 1e-4)
        return poses, status == 2
    want = _relocalize_restated(reg, keypoints, gmap, grid, tau, top_m, planar)
    got = reg.RelocalizePlanar(keypoints, gmap, grid, tau, top_m=top_m, max_iterations=100, convergence=1e-4)
    assert reg.last_status == K.KICP_OK
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]

    # kicp_relocalize on the same inputs still returns what its own restatement gives
    def kinematic(start):
        poses = np.array([reg.ComputeRobotMotion(keypoints, gmap, p, okicp.IDENTITY, tau) for p in start])
        return poses, ~np.isfinite(poses).all(axis=1)
    want = _relocalize_restated(reg, keypoints, gmap, grid, tau, top_m, kinematic)
    got = reg.Relocalize(keypoints, gmap, grid, tau, top_m=top_m)
    assert reg.last_status == K.KICP_OK
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]


def test_recovery(recovery_gpu):
    """the case tests/test_planar_host.py pins: 125 candidates 0.5 m / 6 degrees apart, the truth between the nodes"""
    cfg, gmap, items = recovery_gpu
    reg = K.KinematicRegistration()
    for scan, (keypoints, truth, grid) in enumerate(items):
        for tau in (cfg.first_frame_tau(), 2.0 * cfg.first_frame_tau()):
            n_corr, ssr = reg.ScorePoses(keypoints, gmap, grid, tau)
            cost = cost_of(len(keypoints), n_corr, ssr, tau)
            pose, cand, before, after = reg.RelocalizePlanar(keypoints, gmap, grid, tau, top_m=TOP_M, max_iterations=100, convergence=1e-4)
            assert reg.last_status == K.KICP_OK
            d, yaw = offset(truth, pose)
            print("scan %d tau %.3f: refined from candidate %d, %.4f m and %.4f deg from the truth, cost %.6g -> %.6g" % (scan, tau, cand, d, yaw, before, after))
            assert d < 0.09 and yaw < 0.1
            assert before == cost[cand] and after <= before
            assert cand in np.argsort(cost, kind="stable")[:TOP_M]


@pytest.mark.parametrize("copies", [1, 60])
def test_tie_scenes(handles, copies):
    """tests/tie_cases.py: equidistant candidates, candidates an ulp apart with equal norms, candidates exactly at tau - a wrong pick
    moves a residual by >= 0.3 m, i.e. every shared sum by far more than its last bit"""
    scene = tc.build(copies)
    gmap = K.VoxelHashMap(tc.VS, 100.0, tc.CAP)
    gmap.AddPoints(scene.map_points)
    poses = np.array([IDENT, IDENT])
    want_hits = ~np.isnan(scene.expected[:, 0])
    for reg in handles:
        sums = reg.PlanarSums(scene.queries, gmap, poses, tc.TAU)
        _assert_shared_sums(sums, _pass_sums(reg, scene.queries, gmap, poses, tc.TAU))
        assert sums[0, 0] == want_hits.sum() and np.array_equal(sums[0], sums[1])


def test_map_placement_and_empty_inputs(case1, handles):
    cfg, scans, gmap, keypoints, poses = case1
    tau = cfg.first_frame_tau()
    reg = handles[0]
    dmap = K.VoxelHashMap(cfg.voxel_size, cfg.max_range, cfg.max_points_per_voxel)
    cloud = gmap.Pointcloud()
    assert dmap.UpdateDevice(K.DeviceFrame(cloud), IDENT)  # device-authoritative: the newest state lives in HBM only
    for placed in ("device", "host"):
        if placed == "host":
            dmap.Clear(), dmap.AddPoints(cloud)
        sums = reg.PlanarSums(keypoints, dmap, poses[:7], tau)
        _assert_shared_sums(sums, _pass_sums(reg, keypoints, dmap, poses[:7], tau))
        assert sums[0, 0] > 0.5 * len(keypoints)
    # an update begun and not yet collected is collected by the call (the frame stays alive until then)
    pending = K.DeviceFrame(keypoints)
    dmap.UpdateDevice(K.DeviceFrame(cloud), IDENT)
    dmap.UpdateDeviceBegin(pending, poses[1])
    sums = reg.PlanarSums(keypoints, dmap, poses[:2], tau)
    _assert_shared_sums(sums, _pass_sums(reg, keypoints, dmap, poses[:2], tau))
    dmap.UpdateDeviceBegin(pending, poses[0])
    refined, iterations, status = reg.RefinePosesPlanar(keypoints, dmap, poses[:2], tau, 3, 1e-4)
    again = reg.RefinePosesPlanar(keypoints, dmap, poses[:2], tau, 3, 1e-4)
    assert np.array_equal(refined, again[0]) and (iterations > 0).all()
    # an empty map, an empty frame, no poses: zeros and no launch; a refinement returns the poses with status 2
    empty = K.VoxelHashMap(1.0, 100.0, 20)
    for frame, vmap in ((keypoints, empty), (np.zeros((0, 3)), gmap)):
        sums = reg.PlanarSums(frame, vmap, poses[:7], tau)
        assert sums.shape == (7, 8) and not sums.any() and reg.get_option("score_launches") == 0
        refined, iterations, status = reg.RefinePosesPlanar(frame, vmap, poses[:7], tau)
        assert np.array_equal(refined, poses[:7]) and not iterations.any() and (status == 2).all()
    assert reg.PlanarSums(keypoints, gmap, np.zeros((0, 7)), tau).shape == (0, 8)
    refined, iterations, status = reg.RefinePosesPlanar(keypoints, gmap, np.zeros((0, 7)), tau)
    assert refined.shape == (0, 7) and iterations.shape == (0,) and status.shape == (0,)
    far = K.planar_grid(syn.pose_mul(poses[0], syn.planar_pose(500.0, 0.0, 0.0)), 0.25, 0.25, 0.0, 0.25, 0.25, 0.0)
    pose, cand, before, after = reg.RelocalizePlanar(keypoints, gmap, far, tau, top_m=4)
    assert reg.last_status == K.KICP_WARN_NO_CORRESPONDENCES and cand == 0 and np.array_equal(pose, far[0]) and before == tau * tau == after


def test_errors(case1):
    cfg, scans, gmap, keypoints, poses = case1
    tau = cfg.first_frame_tau()
    reg = K.KinematicRegistration()
    lib = K.lib()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    frame = np.ascontiguousarray(keypoints[:64])
    q = np.ascontiguousarray(poses[:2])
    out_sums, out_poses, its, status = np.zeros(16), np.zeros(14), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    fp, qp, sp, pp = (a.ctypes.data_as(dp) for a in (frame, q, out_sums, out_poses))
    itp, stp = its.ctypes.data_as(ip), status.ctypes.data_as(ip)
    # null pointers
    for args in ((None, gmap._h, fp, 64, qp, 2, tau, sp), (reg._h, None, fp, 64, qp, 2, tau, sp), (reg._h, gmap._h, None, 64, qp, 2, tau, sp),
                 (reg._h, gmap._h, fp, 64, None, 2, tau, sp), (reg._h, gmap._h, fp, 64, qp, 2, tau, None)):
        assert lib.kicp_planar_sums(*args) == K.KICP_ERR_ARG
        assert b"null argument" in lib.kicp_last_error()
    assert lib.kicp_planar_sums_device(reg._h, gmap._h, None, 64, qp, 2, tau, sp) == K.KICP_ERR_ARG
    assert lib.kicp_refine_poses_planar(reg._h, gmap._h, fp, 64, None, 2, tau, 5, 1e-4, pp, itp, stp) == K.KICP_ERR_ARG
    assert lib.kicp_refine_poses_planar(reg._h, gmap._h, fp, 64, qp, 2, tau, 5, 1e-4, None, itp, stp) == K.KICP_ERR_ARG
    assert lib.kicp_refine_poses_planar_device(reg._h, gmap._h, None, 64, qp, 2, tau, 5, 1e-4, pp, itp, stp) == K.KICP_ERR_ARG
    assert lib.kicp_relocalize_planar(reg._h, gmap._h, fp, 64, qp, 2, tau, 2, 5, 1e-4, None, None, None, None) == K.KICP_ERR_ARG
    # documented limits (checked before anything is read: the arrays need not be that long)
    assert lib.kicp_planar_sums(reg._h, gmap._h, fp, 64, qp, (1 << 24) + 1, tau, sp) == K.KICP_ERR_CAPACITY
    assert lib.kicp_planar_sums(reg._h, gmap._h, fp, 0x7FFFFFF0 // 3 + 1, qp, 2, tau, sp) == K.KICP_ERR_CAPACITY
    assert lib.kicp_refine_poses_planar(reg._h, gmap._h, fp, 64, qp, (1 << 24) + 1, tau, 5, 1e-4, pp, itp, stp) == K.KICP_ERR_CAPACITY
    assert lib.kicp_refine_poses_planar(reg._h, gmap._h, fp, 0x7FFFFFF0 // 3 + 1, qp, 2, tau, 5, 1e-4, pp, itp, stp) == K.KICP_ERR_CAPACITY
    # the refinement's own limits
    for max_iterations, convergence in ((0, 1e-4), (-3, 1e-4), (5, -1e-9), (5, float("nan"))):
        assert lib.kicp_refine_poses_planar(reg._h, gmap._h, fp, 64, qp, 2, tau, max_iterations, convergence, pp, itp, stp) == K.KICP_ERR_ARG
        assert b"max_iterations" in lib.kicp_last_error()
        assert lib.kicp_relocalize_planar(reg._h, gmap._h, fp, 64, qp, 2, tau, 2, max_iterations, convergence, pp, None, None, None) == K.KICP_ERR_ARG
    # a multi-GPU exchange attached to the handle: per device only, in kicp_score_poses' words
    sharded = K.KinematicRegistration()
    sharded.set_allreduce(lambda ptr, count, stream: None)
    for call in (lambda: sharded.PlanarSums(keypoints, gmap, poses[:2], tau), lambda: sharded.RefinePosesPlanar(keypoints, gmap, poses[:2], tau),
                 lambda: sharded.RelocalizePlanar(keypoints, gmap, poses[:2], tau)):
        with pytest.raises(K.KicpError) as e:
            call()
        assert e.value.code == K.KICP_ERR_ARG and "detach the multi-GPU exchange first" in str(e.value)
    # the handle is as good as before
    assert reg.PlanarSums(keypoints, gmap, poses[:2], tau)[0, 0] > 0
    refined, iterations, status = reg.RefinePosesPlanar(keypoints, gmap, poses[:2], tau, 2, 0.0)
    assert (iterations == 2).all() and (status == 1).all()
