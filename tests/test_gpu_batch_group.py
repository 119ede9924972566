"""kicp_register_device_batch with SEVERAL SCANS PER LAUNCH (option "batch_group" = G: the passes of up to G scans share one
dispatch of k_pass_gather32_jobs on a 2-D grid, batch_queues / G queues; kicp_reg_queues.hip run_batch_groups): every pose and
every iteration count bit-equal to the same batch registered strictly one scan after the other ("batch_queues" 0), for G = 1 (a
launch per scan and pass), 2, 4 and 8, on a small map.  The one-scan-at-a-time result of a case is computed once and shared by
the four values of G."""
import os

import numpy as np
import pytest

import kinematic_icp_amd as K
from checkers import okicp
from kinematic_icp_amd import synthetic as syn

pytestmark = pytest.mark.gpu
I = okicp.IDENTITY
CFG = dict(max_num_iteration=10, convergence_criterion=1e-3, max_num_threads=1, use_adaptive_odometry_regularization=True,
           fixed_regularization=0.0)
# one lane per query and no small-scan kernels: every scan takes the build of the pass kernel that the job list serves; eight scans
# in flight, so that G = 8 is one lane with eight jobs, G = 4 two lanes, G = 2 four
GROUPED = {"batch_queues": 8, "batch_threads": 0, "lanes_per_query": 1, "small": 0}
PLAIN = {"batch_resident": 0, "batch_queues": 0, "batch_threads": 0, "lanes_per_query": 1, "small": 0}
GROUPS = [1, 2, 4, 8]


def _reg(options, **cfg):
    reg = K.KinematicRegistration(**cfg)
    for k, v in options.items():
        reg.set_option(k, v)
    return reg


class World:
    def __init__(self):
        rng = np.random.default_rng(29)
        mp = np.concatenate([rng.uniform(-40, 40, (60000, 2)), rng.uniform(0, 0.05, (60000, 1))], 1)  # a noisy ground plane: full voxels
        self.map = K.VoxelHashMap(1.0, 100.0, 20)
        self.map.AddPoints(mp)
        self.src = self.map.Pointcloud()[:20000]
        self.frames = {}
        self.want = {}

    def frame(self, n, shift=0.0, start=0):
        key = (n, shift, start)
        if key not in self.frames:
            self.frames[key] = K.DeviceFrame(self.src[start:start + n] - np.array([shift, 0.0, 0.0]), device=0)
        return self.frames[key]

    def nothing(self, n):  # a scan without a single correspondence
        key = (n, "nothing")
        if key not in self.frames:
            self.frames[key] = K.DeviceFrame(np.full((n, 3), 400.0), device=0)
        return self.frames[key]

    def plain(self, name, dev, lasts, rels, tau=0.5, options={}, **cfg):
        """the batch one scan after the other: (poses, iterations, status), computed once per case"""
        if name not in self.want:
            reg = _reg(dict(PLAIN, **options), **dict(CFG, **cfg))
            b = reg.prepare_batch(dev, lasts, rels)
            poses = reg.ComputeRobotMotionBatch(b, self.map, tau).copy()
            assert reg.get_option("batch_queue_passes") == 0.0
            self.want[name] = (poses, list(b.iterations), reg.last_status)
        return self.want[name]


@pytest.fixture(scope="module")
def world():
    return World()


def _grouped(world, name, group, dev, lasts, rels, calls=2, options={}, **cfg):
    want, want_it, status = world.plain(name, dev, lasts, rels, options=options, **cfg)
    reg = _reg(dict(GROUPED, batch_group=group, **options), **dict(CFG, **cfg))
    b = reg.prepare_batch(dev, lasts, rels)
    for _ in range(calls):  # (the second call runs on the lanes' buffers as the first one left them)
        got = reg.ComputeRobotMotionBatch(b, world.map, 0.5).copy()
        assert np.array_equal(got, want, equal_nan=True) and list(b.iterations) == want_it
        assert reg.last_status == status
    assert reg.get_option("batch_queue_passes") >= calls * len(dev)
    assert (reg.get_option("batch_group_launches") > 0) == (group > 1)
    if group > 1:  # ... and went out as hand-written packets on the lanes' own queues (all but a lane's first after its buffers were set up)
        assert reg.get_option("batch_group_aql_launches") >= max(1, reg.get_option("batch_group_launches") - 8)
    return reg, b, want_it


def _poses(count):
    return [syn.planar_pose(0.01 * i, 0.0, 0.001 * i) for i in range(count)], [syn.planar_pose(-0.004 * i, 0.0, 0.0005) for i in range(count)]


@pytest.mark.parametrize("group", GROUPS)
def test_a_batch_whose_length_is_no_multiple_of_the_group(world, group):
    count = 19
    dev = [world.frame(9000 + 500 * (i % 5), 0.01 * (i % 4)) for i in range(count)]
    lasts, rels = _poses(count)
    reg, b, want_it = _grouped(world, "odd", group, dev, lasts, rels)
    if group > 1:  # fewer dispatches than passes: the jobs shared launches
        assert reg.get_option("batch_group_launches") < reg.get_option("batch_queue_passes")


@pytest.mark.parametrize("group", GROUPS)
def test_scans_of_different_sizes_in_one_group(world, group):
    """4 097 points = 17 workgroups, 8 193 = 33 (a second group of ONE workgroup), 20 000 = 79: the launch's grid is the largest
    job's, the others' spare workgroups leave at once, and every job's reduction goes by its own workgroup count"""
    sizes = [4097, 8193, 20000, 12000, 8193, 4097, 19999, 8192] * 2 + [8193]
    dev = [world.frame(k, 0.01 * (i % 3), start=7 * i) for i, k in enumerate(sizes)]
    lasts, rels = _poses(len(sizes))
    _grouped(world, "sizes", group, dev, lasts, rels)


@pytest.mark.parametrize("group", GROUPS)
def test_scans_that_converge_at_once_next_to_scans_that_go_on(world, group):
    """source == map points at the identity: one iteration; scans that start from poses a little off: two to ten (on this flat map
    an odometry guess with 0.05 m / 0.5 deg of extra error alone converges at once - the adaptive regularisation trusts it - so the
    scans that have to go on are made this way) - the scans that go on are regrouped with fresh ones"""
    count = 18
    off = [i % 3 == 1 or i == 6 for i in range(count)]
    dev = [world.frame(9000 + 1000 * (i % 3), 0.08 if off[i] and i % 2 else 0.0) for i in range(count)]
    far_lasts, far_rels = _poses(8)
    lasts = [far_lasts[1 + i % 7] if off[i] else I for i in range(count)]
    rels = [far_rels[1 + i % 7] if off[i] else I for i in range(count)]
    reg, b, want_it = _grouped(world, "convergence", group, dev, lasts, rels)
    assert want_it.count(1) >= 10 and sum(k >= 2 for k in want_it) >= 5 and max(want_it) >= 4


@pytest.mark.parametrize("group", GROUPS)
def test_a_scan_without_correspondences_and_a_single_iteration(world, group):
    count = 17
    dev = [world.frame(10000, 0.02 * (i % 4)) for i in range(count)]
    dev[6] = world.nothing(9000)
    lasts, rels = _poses(count)
    reg, b, want_it = _grouped(world, "nan", group, dev, lasts, rels)
    want = world.want["nan"][0]
    assert np.isnan(want[6]).any() and want_it[6] == 10 and reg.last_status == K.KICP_WARN_NO_CORRESPONDENCES
    _, _, one_it = _grouped(world, "nan_one_iteration", group, dev, lasts, rels, max_num_iteration=1)
    assert set(one_it) == {1}


@pytest.mark.parametrize("group", GROUPS)
def test_a_small_scan_keeps_its_own_kernel_inside_a_grouped_batch(world, group):
    """the small-scan kernels on, sub-lanes per query by scan size: scans beyond 32 768 points share launches, the others - one wave
    per query up to 4 096 points, two sub-lanes per query at 20 000 - go out alone, pass by pass, between the groups"""
    count = 17
    big = np.concatenate([world.src, world.src[:14000] + np.array([0.0, 0.0, 0.001])])  # 34 000 points
    dev = [K.DeviceFrame(big[:33000 + 250 * (i % 4)] - np.array([0.01 * (i % 3), 0.0, 0.0]), device=0) for i in range(count)]
    dev[5] = world.frame(4096, 0.03)
    dev[11] = world.frame(700, 0.02)
    dev[12] = world.frame(20000, 0.02)
    lasts, rels = _poses(count)
    reg, b, want_it = _grouped(world, "mixed_kernels", group, dev, lasts, rels, options={"small": 1, "lanes_per_query": 0})
    if group > 1:
        assert reg.get_option("batch_group_launches") >= 2 * 14 / group


@pytest.mark.parametrize("group", GROUPS)
def test_a_changed_configuration_between_two_calls_on_one_handle(world, group):
    count = 17
    dev = [world.frame(9500, 0.02 * (i % 5)) for i in range(count)]
    far_lasts, far_rels = _poses(8)
    lasts = [far_lasts[1 + i % 7] if i % 2 else I for i in range(count)]
    rels = [far_rels[1 + i % 7] if i % 2 else I for i in range(count)]  # (scans 0 and 10: source == map points at the identity, one iteration)
    reg, b, want_it = _grouped(world, "reconfigure_before", group, dev, lasts, rels, calls=1)
    want, want_it3, _ = world.plain("reconfigure_after", dev, lasts, rels, max_num_iteration=3, convergence_criterion=0.0)
    reg.max_num_iterations_, reg.convergence_criterion_ = 3, 0.0  # (every scan now runs exactly three iterations)
    got = reg.ComputeRobotMotionBatch(b, world.map, 0.5).copy()
    assert np.array_equal(got, want, equal_nan=True) and list(b.iterations) == want_it3 and set(want_it3) == {3} and min(want_it) == 1


@pytest.mark.parametrize("group", GROUPS)
def test_a_batch_too_short_for_the_mode(world, group):
    dev = [world.frame(9000, 0.01 * i) for i in range(3)]
    lasts, rels = _poses(3)
    want, want_it, _ = world.plain("short", dev, lasts, rels)
    reg = _reg(dict(GROUPED, batch_group=group), **CFG)
    b = reg.prepare_batch(dev, lasts, rels)
    got = reg.ComputeRobotMotionBatch(b, world.map, 0.5).copy()
    assert np.array_equal(got, want) and list(b.iterations) == want_it
    assert reg.get_option("batch_queue_passes") == 0.0 and reg.get_option("batch_group_launches") == 0.0


@pytest.mark.parametrize("group", [2, 8])
def test_a_sharded_batch_keeps_the_launch_per_scan(world, group):
    """the shared segment attached (a world of one rank): the lanes' exchanges are per scan and pass, so the batch takes the
    per-scan path whatever "batch_group" says"""
    count = 17
    dev = [world.frame(9000 + 500 * (i % 5), 0.01 * (i % 4)) for i in range(count)]
    lasts, rels = _poses(count)
    want, want_it, _ = world.plain("sharded", dev, lasts, rels)
    reg = _reg(dict(GROUPED, batch_group=group), **CFG)
    reg.shm_init(1, 0, "kicp_group_%d_%d" % (os.getpid(), group))
    try:
        b = reg.prepare_batch(dev, lasts, rels)
        got = reg.ComputeRobotMotionBatch(b, world.map, 0.5).copy()
        assert np.array_equal(got, want, equal_nan=True) and list(b.iterations) == want_it
        assert reg.get_option("batch_queue_passes") >= count and reg.get_option("batch_group_launches") == 0.0
    finally:
        reg.shm_destroy()
