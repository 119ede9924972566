"""The two paths of the pass kernels' limb split (kicp_pass_fixed.hpp::terms_to_fixed) on the GPU, on the scenes of
tests/terms_paths_cases.py (whose premises() proves on the CPU which queries leave the short path): one lane of a wave, sixteen lanes of
every wave, every lane of one wave and none of the others, every lane, no lane, and the second of two tiles of a workgroup hold a
correspondence whose s.x^2 + s.y^2 is 2^22 or more - source points at about 3 000 m.

The scenes are exact in fp64 (see the cases' module), so for every build of the pass kernel a handle can pick the sums must equal the
oracle's BIT FOR BIT, and with them one another; a batch through the job list returns the bits of the single calls.  At a rotated pose,
where the oracle's own sums round, the builds are held to one another bit for bit and to the oracle within the tolerance of
tests/test_gpu_parity.py.  At the distance where tests/test_gpu_ranges.py finds the accumulation's range error every build still
reports KICP_ERR_CAPACITY, and just inside it they agree on the pose."""
import numpy as np
import pytest

import kinematic_icp_amd as K
import terms_paths_cases as tc
from checkers import okicp
from kinematic_icp_amd import synthetic as syn

pytestmark = pytest.mark.gpu
SUM_RTOL = 1e-10  # tests/test_gpu_parity.py test_pass_sums_match_oracle
FOUR_WAVES = {"small": 0, "lanes_per_query": 1, "latency_kernel": 0}
BUILDS = [  # (tests/test_gpu_mirror_z.py)
    ("four_waves", FOUR_WAVES),                                                    # k_pass_gather32<256, 1, 4, false, false>
    ("latency_build", {"small": 0, "lanes_per_query": 1, "latency_kernel": 2}),   # <256, 1, 2, false, true>
    ("two_sub_lanes", {"small": 0, "lanes_per_query": 2}),                         # <256, 2, 4, true, false>
    ("four_sub_lanes", {"small": 0, "lanes_per_query": 4}),                        # <256, 4, 4, false, false>
    ("k_pass_small", {"small": 1, "small_wave": 0}),
    ("k_pass_wave", {"small": 1, "small_wave": 1}),
]
GROUPED = dict(FOUR_WAVES, batch_queues=8, batch_threads=0, batch_group=4)
SCENES = sorted(tc.BUILDERS)


def _reg(options):
    reg = K.KinematicRegistration()
    for k, v in options.items():
        reg.set_option(k, v)
    return reg


class World:
    """the map on the device and in the oracle, the scenes and the oracle's sums - computed once, never changed"""

    def __init__(self):
        far, near = tc.map_points()
        self.omap = tc.oracle_map()
        self.map = K.VoxelHashMap(tc.VS, tc.MAX_DISTANCE, tc.CAP)
        self.map.AddPoints(np.concatenate([far, near]))
        assert self.map.num_points() == self.omap.num_points() and self.map.check() == 0
        self.scenes, self.want = {}, {}
        for name in SCENES:
            scene = tc.BUILDERS[name]()
            tc.premises(scene, self.omap)
            self.scenes[name] = scene
            self.want[name] = okicp.icp_pass(self.omap, scene.queries, tc.POSE, tc.TAU)[0]
            assert np.array_equal(self.want[name], tc.exact_sums(scene))


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.mark.parametrize("name", SCENES)
def test_every_build_sums_the_oracles_bits(world, name):
    scene = world.scenes[name]
    for build, options in BUILDS:
        reg = _reg(dict(options, pass_tiles=scene.tiles) if build == "four_waves" else options)
        sums = reg.pass_sums(scene.queries, world.map, tc.POSE, tc.TAU)
        assert np.array_equal(sums, world.want[name]), (build, sums - world.want[name])
        idx = reg.pass_correspondences(scene.queries, world.map, tc.POSE, tc.TAU)[0]
        assert (idx >= 0).all(), build


@pytest.mark.parametrize("name", SCENES)
def test_a_rotated_pose_gives_every_build_the_same_bits(world, name):
    """the same images reached through a pose with a yaw: the terms round, the builds must still agree to the bit"""
    scene = world.scenes[name]
    pose = syn.planar_pose(8.0, -4.0, 0.3)
    src = syn.pose_act(syn.pose_inverse(pose), scene.images)
    want, _ = okicp.icp_pass(world.omap, src, pose, tc.TAU)
    assert want[6] == scene.n and want[2] >= tc.SHORT_LIMIT * scene.far.sum()
    first = None
    for build, options in BUILDS:
        sums = _reg(dict(options, pass_tiles=scene.tiles) if build == "four_waves" else options).pass_sums(src, world.map, pose, tc.TAU)
        np.testing.assert_allclose(sums, want, rtol=SUM_RTOL, atol=1e-9)
        if first is None:
            first = sums
        assert np.array_equal(sums, first), build


def test_a_batch_through_the_job_list_returns_the_bits_of_the_single_calls(world):
    """the scenes three times over: eighteen scans, groups of four jobs on two lanes (k_pass_gather32_jobs)"""
    scans = [world.scenes[name].queries for name in SCENES] * 3
    last = syn.pose_mul(tc.POSE, syn.pose_inverse(syn.planar_pose(0.015625, 0.0, 0.0)))
    rel = syn.planar_pose(0.015625, 0.0, 0.0)
    reg = _reg(GROUPED)
    b = reg.prepare_batch([K.DeviceFrame(s, device=0) for s in scans], [last] * len(scans), [rel] * len(scans))
    got = reg.ComputeRobotMotionBatch(b, world.map, tc.TAU).copy()
    assert reg.get_option("batch_group_launches") > 0
    for k, name in enumerate(SCENES):
        single, oreg = _reg(FOUR_WAVES), okicp.KinematicRegistration()
        pose = single.ComputeRobotMotion(scans[k], world.map, last, rel, tc.TAU)
        ref = oreg.ComputeRobotMotion(scans[k], world.omap, last, rel, tc.TAU)
        np.testing.assert_allclose(pose, ref, rtol=0, atol=1e-9)
        assert single.last_stats.iterations == oreg.last_stats.iterations
        for rep in range(3):
            j = k + rep * len(SCENES)
            assert np.array_equal(got[j], pose), (name, rep)
            assert int(b.iterations[j]) == single.last_stats.iterations


def test_the_range_error_comes_out_as_before():
    """tests/test_gpu_ranges.py's distances in a scan of 256 points: a source point 2 960 km out is summed (the general path, one lane),
    one 2 970 km out is KICP_ERR_CAPACITY in every build - never a wrapped sum, never the short path's silence"""
    rng = np.random.default_rng(3)
    base = rng.uniform(-20, 20, (3000, 3)) * np.array([1, 1, 0.1])
    body = base[::3][:255] + rng.normal(0, 0.01, (255, 3))
    for far, ok in ((2.96e6, True), (2.97e6, False)):
        g, o = K.VoxelHashMap(1.0, 1e7, 20), okicp.VoxelHashMap(1.0, 1e7, 20)
        mpts = np.concatenate([base, [[far + 0.01, 0.3, 0.2]]])
        g.AddPoints(mpts), o.AddPoints(mpts)
        frame = np.concatenate([body[:100], [[far, 0.3, 0.2]], body[100:]])
        rel = syn.planar_pose(0.01, 0.0, 0.1 / far)  # (the far point must stay within tau of its map point)
        first = None
        for build, options in BUILDS:
            reg = _reg(options)
            if ok:
                pose = reg.ComputeRobotMotion(frame, g, okicp.IDENTITY, rel, 0.5)
                if first is None:
                    oreg = okicp.KinematicRegistration()
                    ref = oreg.ComputeRobotMotion(frame, o, okicp.IDENTITY, rel, 0.5)
                    np.testing.assert_allclose(pose, ref, rtol=0, atol=1e-6)  # (tests/test_gpu_ranges.py's bound at this distance)
                    assert reg.last_stats.iterations == oreg.last_stats.iterations
                    first = pose
                assert np.array_equal(pose, first), build
            else:
                with pytest.raises(K.KicpError) as e:
                    reg.ComputeRobotMotion(frame, g, okicp.IDENTITY, rel, 0.5)
                assert e.value.code == K.KICP_ERR_CAPACITY, build
