"""Several blocks of 256 queries per workgroup in the one-lane-per-query four-waves build of the pass kernel (option "pass_tiles" =
T: k_pass_gather32<256, 1, 4, false, false>, its EXPORT twin and k_pass_gather32_jobs; kicp_kernels.hpp pass_tiles_loop).  The sums
are exact integers, so every pose, iteration count, status and per-query decision must be bit-equal to one block per workgroup
(T = 1) - in single calls, in batches whose launches mix jobs of different workgroup and tile counts, where only a workgroup's last
tile holds correspondences, where only its last tile leaves the accumulation's range, and under the automatic rule.  Small scans
are forced into that build ("lanes_per_query" 1, "small" 0, "latency_kernel" 0).  The T = 1 result of a case is computed once and
shared by the tile counts."""
import numpy as np
import pytest

import kinematic_icp_amd as K
from checkers import okicp
from kinematic_icp_amd import synthetic as syn

pytestmark = pytest.mark.gpu
I = okicp.IDENTITY
POSE_TOL = 1e-9  # (tests/test_gpu_parity.py)
TAU = 0.5
CFG = dict(max_num_iteration=10, convergence_criterion=1e-3, max_num_threads=1, use_adaptive_odometry_regularization=True,
           fixed_regularization=0.0)
FOUR_WAVES = {"lanes_per_query": 1, "small": 0, "latency_kernel": 0}
PLAIN = dict(FOUR_WAVES, batch_resident=0, batch_queues=0, batch_threads=0)
GROUPED = dict(FOUR_WAVES, batch_queues=8, batch_threads=0)
TILES = [1, 2, 4]
MULTI_ITER_ERROR = syn.planar_pose(0.05, 0.0, np.deg2rad(0.5))  # (bench.py's multi-iteration workload)


def sizes_of(T):
    """up to one block, around T blocks (one full workgroup), T + 1 blocks (the last workgroup has fewer tiles than the others),
    and one point more than 32 workgroups of T blocks (a second group row)"""
    return sorted({1, 255, 256, 257, 256 * T - 1, 256 * T, 256 * T + 1, 256 * (T + 1), 32 * 256 * T + 1})


def _reg(options, **cfg):
    reg = K.KinematicRegistration(**dict(CFG, **cfg))
    for k, v in options.items():
        reg.set_option(k, v)
    return reg


class World:
    def __init__(self):
        rng = np.random.default_rng(29)
        self.map_points = np.concatenate([rng.uniform(-40, 40, (90000, 2)), rng.uniform(0, 0.05, (90000, 1))], 1)  # a noisy ground plane: full voxels
        self.map = K.VoxelHashMap(1.0, 100.0, 20)
        self.map.AddPoints(self.map_points)
        self.src = self.map.Pointcloud()[:40000]  # (the map keeps the points that are not too close to one it holds: about half)
        assert len(self.src) >= 32 * 256 * 4 + 1 + 7 * 18  # the largest scan, from the largest offset scan() takes
        self.omap = None
        self.cache = {}

    def oracle_map(self):
        if self.omap is None:
            self.omap = okicp.VoxelHashMap(1.0, 100.0, 20)
            self.omap.AddPoints(self.map_points)
        return self.omap

    def scan(self, n, i=0):
        """n points of the map, moved a little: registrations of several iterations from `poses(i)`"""
        return self.src[7 * i:7 * i + n] - np.array([0.08 if i % 2 else 0.02, 0.0, 0.0])

    @staticmethod
    def poses(i):
        last = syn.planar_pose(0.01 * (1 + i % 7), 0.0, 0.001 * (1 + i % 7))
        rel = syn.pose_mul(syn.planar_pose(-0.004 * (1 + i % 7), 0.0, 0.0005), MULTI_ITER_ERROR if i % 3 == 0 else I)
        return last, rel

    def single(self, frame, last, rel, tiles, the_map=None):
        """(pose, iterations, status, correspondence indices at the start pose) of one call"""
        reg = _reg(dict(FOUR_WAVES, pass_tiles=tiles))
        m = the_map if the_map is not None else self.map
        pose = reg.ComputeRobotMotion(frame, m, last, rel, TAU)
        it, status = reg.last_stats.iterations, reg.last_status
        index = reg.pass_correspondences(frame, m, syn.pose_mul(last, rel), TAU)[0].copy()
        return pose, it, status, index

    def single_want(self, key, frame, last, rel, the_map=None):
        if key not in self.cache:
            self.cache[key] = self.single(frame, last, rel, 1, the_map)
        return self.cache[key]


@pytest.fixture(scope="module")
def world():
    return World()


def _same(got, want):
    assert np.array_equal(got[0], want[0], equal_nan=True) and got[1] == want[1] and got[2] == want[2]
    assert np.array_equal(got[3], want[3])


@pytest.mark.parametrize("T", TILES)
def test_single_calls_at_each_tile_count(world, T):
    iterations = []
    for k, n in enumerate(sizes_of(T)):
        frame = world.scan(n, k)
        last, rel = world.poses(k)
        want = world.single_want(("single", n, k), frame, last, rel)
        got = world.single(frame, last, rel, T)
        _same(got, want)
        iterations.append(got[1])
        if n > 1:
            assert (got[3] >= 0).sum() > n // 2  # (the scan does have correspondences)
        if n <= 257:
            oreg = okicp.KinematicRegistration(**CFG)
            ref = oreg.ComputeRobotMotion(frame, world.oracle_map(), last, rel, TAU)
            np.testing.assert_allclose(got[0], ref, rtol=0, atol=POSE_TOL, equal_nan=True)
            assert got[1] == oreg.last_stats.iterations
    assert max(iterations) >= 2  # (later passes of a call ran tiled, too)


def _batch_case(world, T):
    """two scans of every size of sizes_of(T), sizes mixed along the batch - a launch of four jobs holds scans of one block (one
    workgroup of one tile, whatever T) next to scans of T, T + 1 and 32 T + 1 blocks - and every third scan with the extra odometry error"""
    sizes = sizes_of(T)
    order = sizes + sizes[::-1]
    order = (order * 2)[:max(len(order), 18)]  # (T = 1 has six sizes; a batch of fewer than 16 scans would not take the queues)
    frames = [K.DeviceFrame(world.scan(n, i), device=0) for i, n in enumerate(order)]
    poses = [world.poses(i) for i in range(len(order))]
    return frames, [p[0] for p in poses], [p[1] for p in poses]


@pytest.mark.parametrize("group", [1, 4])
@pytest.mark.parametrize("T", TILES)
def test_batches_that_mix_workgroup_and_tile_counts(world, T, group):
    key = ("batch", T)
    if key not in world.cache:
        frames, lasts, rels = _batch_case(world, T)
        reg = _reg(dict(PLAIN, pass_tiles=1))
        b = reg.prepare_batch(frames, lasts, rels)
        poses = reg.ComputeRobotMotionBatch(b, world.map, TAU).copy()
        assert reg.get_option("batch_queue_passes") == 0.0
        world.cache[key] = (frames, lasts, rels, poses, list(b.iterations), reg.last_status)
    frames, lasts, rels, want, want_it, status = world.cache[key]
    assert max(want_it) >= 2 and min(want_it) >= 1
    reg = _reg(dict(GROUPED, batch_group=group, pass_tiles=T))
    b = reg.prepare_batch(frames, lasts, rels)
    for _ in range(2):  # (the second call runs on the lanes' buffers as the first one left them)
        got = reg.ComputeRobotMotionBatch(b, world.map, TAU).copy()
        assert np.array_equal(got, want, equal_nan=True) and list(b.iterations) == want_it and reg.last_status == status
    assert reg.get_option("batch_queue_passes") >= 2 * len(frames)
    assert (reg.get_option("batch_group_launches") > 0) == (group > 1)


@pytest.mark.parametrize("T", [2, 4])
def test_correspondences_in_one_tile_only(world, T):
    """a single workgroup of T tiles: only its last tile holds correspondences (waves without a holder in the other tiles; the count
    and |R UnitX|^2 come from the tiles' ballots), only its first, and none at all"""
    far = np.full((256 * (T - 1), 3), 400.0)
    near = world.scan(200, 3)
    last, rel = world.poses(3)
    for name, frame in (("last", np.concatenate([far, near])), ("first", np.concatenate([near, far])), ("none", np.full((256 * T, 3), 400.0))):
        want = world.single_want(("one tile", name, T), frame, last, rel)
        got = world.single(frame, last, rel, T)
        _same(got, want)
        if name == "none":
            assert got[2] == K.KICP_WARN_NO_CORRESPONDENCES and (got[3] < 0).all()
        else:
            assert got[2] == K.KICP_OK and (got[3] >= 0).sum() > 100 and not np.isnan(got[0]).any()
    # the same correspondences wherever they stand in the scan: the same exact sums, the same pose
    assert np.array_equal(world.cache[("one tile", "last", T)][0], world.cache[("one tile", "first", T)][0])


@pytest.mark.parametrize("T", TILES)
def test_a_range_error_in_the_last_tile(world, T):
    """a term at or beyond 2^43 (a source point ~2 970 km out: s_x^2 + s_y^2, tests/test_gpu_ranges.py) in the workgroup's last tile
    only: KICP_ERR_CAPACITY, never a wrapped sum"""
    if "far map" not in world.cache:
        rng = np.random.default_rng(3)
        base = rng.uniform(-20, 20, (3000, 3)) * np.array([1, 1, 0.1])
        g = K.VoxelHashMap(1.0, 1e7, 20)
        g.AddPoints(np.concatenate([base, [[2.97e6 + 0.01, 0.3, 0.2], [2890.0 + 0.01, 0.3, 0.2]]]))
        world.cache["far map"] = (g, base, rng.normal(0, 0.01, (1000, 3)))
    g, base, noise = world.cache["far map"]
    n_before = 256 * (T - 1) + 100
    body = (np.tile(base[::3], (2, 1))[:n_before] + np.tile(noise, (2, 1))[:n_before])
    for far, ok in ((2890.0, True), (2.97e6, False)):
        frame = np.concatenate([body, [[far, 0.3, 0.2]]])
        rel = syn.planar_pose(0.01, 0.0, min(1e-4, 0.1 / far))  # (the far point must stay within tau of its map point)
        reg = _reg(dict(FOUR_WAVES, pass_tiles=T))
        if ok:
            want = world.single_want(("in range", T), frame, I, rel, g)
            pose = reg.ComputeRobotMotion(frame, g, I, rel, TAU)
            assert np.array_equal(pose, want[0]) and reg.last_stats.iterations == want[1]
        else:
            with pytest.raises(K.KicpError) as e:
                reg.ComputeRobotMotion(frame, g, I, rel, TAU)
            assert e.value.code == K.KICP_ERR_CAPACITY


@pytest.mark.parametrize("n", [300, 32 * 256 * 4 + 1])
def test_the_automatic_rule_changes_no_bit(world, n):
    frame = world.scan(n, 1)
    last, rel = world.poses(1)
    results = {T: world.single(frame, last, rel, T) for T in (0, 1, 2, 4)}
    for T in (0, 2, 4):
        _same(results[T], results[1])
    assert results[0][1] >= 2


def test_the_option_is_clamped_read_back_and_cloned():
    reg = K.KinematicRegistration(**CFG)
    assert reg.get_option("pass_tiles") == 0.0  # automatic
    for value, want in ((1, 1), (2, 2), (3, 2), (4, 4), (9, 4), (-1, 0), (0, 0)):
        reg.set_option("pass_tiles", value)
        assert reg.get_option("pass_tiles") == want
    reg.set_option("pass_tiles", 2)
    assert reg.copy().get_option("pass_tiles") == 2.0
