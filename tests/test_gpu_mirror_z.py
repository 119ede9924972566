"""The second word of a mirror point - z as a float, an empty slot as 4 294 901 760.0f (kicp_common.hpp::MirrorPoint) - through every
build of the pass kernel a handle can pick, on the scenes of tests/mirror_z_cases.py, whose premises() proves on the CPU that each regime
is entered: buckets of 1, 19 and 20 points, two-trip buckets of 20, 21 and 40, points with mirror z 0 and 65 535 (also in a trip's last
slot), an empty own voxel next to a bucket of one, buckets emptied and re-used on the host and on the device.

Every map is built twice, on the host and through UpdateDevice, and looked at after the steps the scene names: the table invariants
(check(), which holds the mirror's words to the format), the buckets point for point, then for each build the chosen correspondence
index for index against the oracle's association (kicp_pass_correspondences: the same queries accepted, the very same map point, the
pool index naming that point's slot) and the pass sums against the oracle's (tests/test_gpu_parity.py test_pass_sums_match_oracle).
A batch of the scans through the job list returns the bits of the single calls.  The oracle's results are computed once per scene."""
import numpy as np
import pytest

import kinematic_icp_amd as K
import mirror_z_cases as mc
from checkers import okicp
from mapdev_ref import bucket_sorted

pytestmark = pytest.mark.gpu
I = mc.IDENTITY
TAU = mc.TAU
SUM_RTOL = 1e-10  # tests/test_gpu_parity.py test_pass_sums_match_oracle
FOUR_WAVES = {"small": 0, "lanes_per_query": 1, "latency_kernel": 0}
BUILDS = [
    ("four_waves", FOUR_WAVES),                                                    # k_pass_gather32<256, 1, 4, false, false>
    ("latency_build", {"small": 0, "lanes_per_query": 1, "latency_kernel": 2}),   # <256, 1, 2, false, true>
    ("two_sub_lanes", {"small": 0, "lanes_per_query": 2}),                         # <256, 2, 4, true, false>
    ("four_sub_lanes", {"small": 0, "lanes_per_query": 4}),                        # <256, 4, 4, false, false>
    ("k_pass_small", {"small": 1, "small_wave": 0}),
    ("k_pass_wave", {"small": 1, "small_wave": 1}),
]
GROUPED = dict(FOUR_WAVES, batch_queues=8, batch_threads=0, batch_group=4)
SCENES = sorted(mc.BUILDERS)
ROUTES = ["host", "device"]


def _reg(options):
    reg = K.KinematicRegistration()
    for k, v in options.items():
        reg.set_option(k, v)
    return reg


class World:
    """the scenes, their states on the CPU and the oracle's answers - computed once, never changed"""

    def __init__(self):
        self.wall = mc.wall_render()
        self.scenes, self.states, self._want = {}, {}, {}
        for name in SCENES:
            scene = mc.BUILDERS[name]()
            self.scenes[name] = scene
            self.states[name] = mc.replay(scene, self.wall)
            mc.premises(scene, self.states[name])

    def want(self, name, state):
        if (name, state) not in self._want:
            scene = self.scenes[name]
            acc, nn, d, rank = mc.expected(scene, self.states[name], state)
            sums, _ = okicp.icp_pass(self.states[name][state][1], scene.queries[state], I, TAU)
            assert sums[6] == acc.sum()
            self._want[(name, state)] = (acc, nn, d, rank, sums)
        return self._want[(name, state)]


@pytest.fixture(scope="module")
def world():
    return World()


def walk(world, name, route):
    """build the scene's map step by step on `route`; yields (state, map) wherever the scene wants a look, after holding the map's
    invariants and its buckets - points and their order - to the model"""
    import view_cases as vc
    scene = world.scenes[name]
    gmap = K.VoxelHashMap(mc.VS, scene.max_distance, scene.cap)
    for k, step in enumerate(scene.steps):
        if step[0] == "update":
            _, points, origin = step
            if route == "host":
                gmap.AddPoints(points)
                gmap.RemovePointsFarFromLocation(origin)
            else:
                assert gmap.UpdateDevice(K.DeviceFrame(points - origin), np.concatenate([[0.0, 0.0, 0.0, 1.0], origin]))
        else:
            cfg = vc.WALL_CFG
            view = K.DepthView(cfg["res"], cfg["window"], cfg["min_rays"], cfg["max_ray"], cfg["margin"], cfg["margin_per_metre"])
            assert view.render(world.wall[0], vc.IDENTITY, vc.ORIGIN) == world.wall[3]
            assert gmap.RemoveSeenThrough(view)[3] >= 1
        if k + 1 in scene.looks:
            state = scene.looks[k + 1]
            model = world.states[name][state][0]
            assert gmap.check() == 0
            assert np.array_equal(bucket_sorted(gmap.Pointcloud(), mc.VS), bucket_sorted(model.points(), mc.VS))
            yield state, gmap
            assert gmap.check() == 0


def _check_build(options, gmap, cap, queries, want):
    acc, onn, od, rank, osums = want
    reg = _reg(options)
    idx, d2, nn = reg.pass_correspondences(queries, gmap, I, TAU)
    np.testing.assert_array_equal(idx >= 0, acc)                     # the same queries have a correspondence ...
    np.testing.assert_array_equal(nn[acc], onn[acc])                 # ... to the very same map point, bit for bit ...
    np.testing.assert_array_equal(np.sqrt(d2[acc]), od[acc])
    np.testing.assert_array_equal(idx[acc] % cap, rank[acc])         # ... which sits in that slot of its bucket
    assert np.all(idx[~acc] == -1) and np.all(d2[~acc] == np.finfo(np.float64).max) and not nn[~acc].any()
    same_voxel = {}
    for i in np.flatnonzero(acc):  # one bucket per voxel: the index names the bucket as well
        assert same_voxel.setdefault(tuple(np.floor(onn[i] / mc.VS)), idx[i] // cap) == idx[i] // cap
    sums = reg.pass_sums(queries, gmap, I, TAU)
    assert sums[6] == osums[6]
    np.testing.assert_allclose(sums, osums, rtol=SUM_RTOL, atol=1e-9)
    return idx, sums


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", SCENES)
def test_every_build_picks_the_oracles_points(world, name, route):
    scene = world.scenes[name]
    looks = 0
    for state, gmap in walk(world, name, route):
        q = scene.queries[state]
        first = None
        for build, options in BUILDS:
            idx, sums = _check_build(options, gmap, scene.cap, q, world.want(name, state))
            if first is None:
                first = (idx, sums)
            assert np.array_equal(idx, first[0]), build  # (the builds agree on the index)
        looks += 1
    assert looks == len(scene.looks)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", SCENES)
def test_a_batch_returns_the_bits_of_the_single_calls(world, name, route):
    """eighteen scans per state - the whole scan, every other query, and scans that end inside a wave, three times over: two lanes
    need two groups of four jobs each before a batch goes through the job list's kernel"""
    scene = world.scenes[name]
    for state, gmap in walk(world, name, route):
        q = scene.queries[state]
        scans = ([q, np.ascontiguousarray(q[::2])] + [np.ascontiguousarray(q[:n]) for n in mc.LENGTHS]) * 3
        frames = [K.DeviceFrame(s, device=0) for s in scans]
        reg = _reg(GROUPED)
        b = reg.prepare_batch(frames, [I] * len(scans), [I] * len(scans))
        got = reg.ComputeRobotMotionBatch(b, gmap, TAU).copy()
        assert reg.get_option("batch_group_launches") > 0
        single = _reg(FOUR_WAVES)
        singles = []
        for s in scans[:6]:  # (every distinct scan once)
            pose = single.ComputeRobotMotion(s, gmap, I, I, TAU)
            singles.append((pose.copy(), single.last_stats.iterations))
        for k in range(len(scans)):
            assert np.array_equal(got[k], singles[k % 6][0], equal_nan=True), (state, k)
            assert int(b.iterations[k]) == singles[k % 6][1]
