"""The lending round of the one-lane-per-query pass kernels (kicp_kernels.hpp::gather32_pass) on the scenes of tests/lend_round_cases.py,
whose premises() replays the first lending round on the CPU: no idle lane (the round that lends nothing), one idle lane beside a lane
with two voxels to spare, more jobs than idle lanes, more than kLendJobs = 32 jobs in every wave of a 256-query scan, a lent visit that
finds nothing, one that finds the winner, and one that ties the owner's own candidate - where the earlier visiting order, the owner's,
must win as in the reference.

Every build of the pass kernel a handle can pick (the lending ones and the others alike) must return the oracle's correspondence for
every query - the same queries accepted, the very same map point, the same distance - and the builds' sums must be equal bit for bit; a
batch through the job list returns the bits of the single calls.  The oracle's answers are computed once per scene."""
import numpy as np
import pytest

import kinematic_icp_amd as K
import lend_round_cases as lc
from checkers import okicp

pytestmark = pytest.mark.gpu
I = lc.I
SUM_RTOL = 1e-10  # tests/test_gpu_parity.py test_pass_sums_match_oracle
FOUR_WAVES = {"small": 0, "lanes_per_query": 1, "latency_kernel": 0}
BUILDS = [  # (tests/test_gpu_mirror_z.py)
    ("four_waves", FOUR_WAVES),                                                    # k_pass_gather32<256, 1, 4, false, false>: lends
    ("latency_build", {"small": 0, "lanes_per_query": 1, "latency_kernel": 2}),   # <256, 1, 2, false, true>
    ("two_sub_lanes", {"small": 0, "lanes_per_query": 2}),                         # <256, 2, 4, true, false>
    ("four_sub_lanes", {"small": 0, "lanes_per_query": 4}),                        # <256, 4, 4, false, false>
    ("k_pass_small", {"small": 1, "small_wave": 0}),                               # (one lane per query: lends)
    ("k_pass_wave", {"small": 1, "small_wave": 1}),
]
GROUPED = dict(FOUR_WAVES, batch_queues=8, batch_threads=0, batch_group=4)
SCENES = sorted(lc.BUILDERS)


def _reg(options):
    reg = K.KinematicRegistration()
    for k, v in options.items():
        reg.set_option(k, v)
    return reg


class World:
    def __init__(self):
        self.scenes, self.maps, self.want = {}, {}, {}
        for name in SCENES:
            scene = lc.BUILDERS[name]()
            omap = lc.oracle_map(scene)
            lc.premises(scene, omap)
            gmap = K.VoxelHashMap(lc.VS, 100.0, lc.CAP)
            gmap.AddPoints(scene.map_points)
            assert gmap.check() == 0 and gmap.num_points() == omap.num_points()
            acc, nn, d = okicp.associate(omap, scene.queries, I, lc.TAU)
            sums, _ = okicp.icp_pass(omap, scene.queries, I, lc.TAU)
            self.scenes[name], self.maps[name], self.want[name] = scene, (gmap, omap), (acc, nn, d, sums)


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.mark.parametrize("name", SCENES)
def test_every_build_returns_the_oracles_correspondences(world, name):
    scene, (gmap, _), (acc, onn, od, osums) = world.scenes[name], world.maps[name], world.want[name]
    first = None
    for build, options in BUILDS:
        reg = _reg(options)
        idx, d2, nn = reg.pass_correspondences(scene.queries, gmap, I, lc.TAU)
        np.testing.assert_array_equal(idx >= 0, acc, err_msg=build)
        np.testing.assert_array_equal(nn[acc], onn[acc], err_msg=build)  # the very same map point: a tie goes to the earlier visit
        np.testing.assert_array_equal(np.sqrt(d2[acc]), od[acc], err_msg=build)
        sums = reg.pass_sums(scene.queries, gmap, I, lc.TAU)
        assert sums[6] == osums[6] == scene.n
        np.testing.assert_allclose(sums, osums, rtol=SUM_RTOL, atol=1e-9)
        if first is None:
            first = (idx, sums)
        assert np.array_equal(idx, first[0]) and np.array_equal(sums, first[1]), build


def test_a_batch_through_the_job_list_returns_the_bits_of_the_single_calls(world):
    """the scenes on M4 and the scenes on M3, each set three times over in a batch of its own: groups of four jobs (k_pass_gather32_jobs)"""
    for names in ([n for n in SCENES if len(world.scenes[n].map_points) == 4], [n for n in SCENES if len(world.scenes[n].map_points) == 3]):
        gmap, omap = world.maps[names[0]]
        scans = [world.scenes[n].queries for n in names] * 6
        reg = _reg(GROUPED)
        b = reg.prepare_batch([K.DeviceFrame(s, device=0) for s in scans], [I] * len(scans), [I] * len(scans))
        got = reg.ComputeRobotMotionBatch(b, gmap, lc.TAU).copy()
        assert reg.get_option("batch_group_launches") > 0
        for k, name in enumerate(names):
            single, oreg = _reg(FOUR_WAVES), okicp.KinematicRegistration()
            pose = single.ComputeRobotMotion(scans[k], gmap, I, I, lc.TAU)
            ref = oreg.ComputeRobotMotion(scans[k], omap, I, I, lc.TAU)
            np.testing.assert_allclose(pose, ref, rtol=0, atol=1e-9)
            assert single.last_stats.iterations == oreg.last_stats.iterations
            for rep in range(6):
                j = k + rep * len(names)
                assert np.array_equal(got[j], pose), (name, rep)
                assert int(b.iterations[j]) == single.last_stats.iterations
