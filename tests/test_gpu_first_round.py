"""The first visiting round of the one-lane-per-query four-waves pass kernel (kicp_kernels.hpp: the first round of gather32_pass;
kicp_pass_visit.hpp: visit_first, process_trip FRESH - k_pass_gather32<256, 1, 4, false, false>, its EXPORT twin, k_pass_gather32_jobs) on the scenes of
tests/first_round_cases.py, whose premises() proves on the CPU that each regime is entered: an empty own voxel next to occupied ones,
the nearest point across a face with exact ties, buckets of two trips, own-voxel candidates around tau and around the kernel's bound,
near-equal candidates, scans that leave lanes of the last wave without a query, queries without any entry.

Every case runs as a single call, as a batch (the jobs kernel) at 1, 2 and 4 tiles per workgroup and through
kicp_pass_correspondences, and is held to the oracle: the correspondences query for query (okicp.associate), the first pass's sums
(okicp.icp_pass) and the poses by the suite's parity rule (1e-9, tests/test_gpu_parity.py).  The latency-oriented build, which has no
such round, must agree bit for bit.  Small scans are forced into the four-waves build ("lanes_per_query" 1, "small" 0,
"latency_kernel" 0).  The oracle's results of a scan are computed once and shared."""
import numpy as np
import pytest

import first_round_cases as fc
import kinematic_icp_amd as K
from checkers import okicp

pytestmark = pytest.mark.gpu
I = okicp.IDENTITY
POSE_TOL = 1e-9  # (tests/test_gpu_parity.py)
TAU = fc.TAU
CFG = dict(max_num_iteration=10, convergence_criterion=1e-3, max_num_threads=1, use_adaptive_odometry_regularization=True,
           fixed_regularization=0.0)
FOUR_WAVES = {"lanes_per_query": 1, "small": 0, "latency_kernel": 0}
LATENCY = {"lanes_per_query": 1, "small": 0, "latency_kernel": 2}
GROUPED = dict(FOUR_WAVES, batch_queues=8, batch_threads=0)
TILES = [1, 2, 4]
CASES = ["halo", "across", "beyond", "near", "mixed", "deep"]


def _reg(options, **cfg):
    reg = K.KinematicRegistration(**dict(CFG, **cfg))
    for k, v in options.items():
        reg.set_option(k, v)
    return reg


class World:
    def __init__(self):
        self.scenes = {}
        for scene in (fc.build(), fc.build_deep()):
            omap = fc.oracle_map(scene)
            fc.premises(scene, omap)
            gmap = K.VoxelHashMap(fc.VS, 100.0, scene.cap)
            gmap.AddPoints(scene.map_points)
            assert gmap.num_points() == len(scene.map_points)
            for name in scene.frames:
                self.scenes[name] = (scene, gmap, omap)
        self._want = {}

    def frame(self, name, n=None):
        f = self.scenes[name][0].frames[name]
        return f if n is None else f[:n]

    def want(self, name, n=None):
        """the oracle on scan `name` (its first n points): (accepted, targets, distances, first pass's sums, pose, iterations)"""
        if (name, n) not in self._want:
            _, _, omap = self.scenes[name]
            f = self.frame(name, n)
            acc, nn, d = okicp.associate(omap, f, I, TAU)
            sums, _ = okicp.icp_pass(omap, f, I, TAU)
            assert sums[6] == acc.sum()
            oreg = okicp.KinematicRegistration(**CFG)
            pose = oreg.ComputeRobotMotion(f, omap, I, I, TAU)
            self._want[(name, n)] = (acc, nn, d, sums, pose, oreg.last_stats.iterations)
        return self._want[(name, n)]


@pytest.fixture(scope="module")
def world():
    return World()


def _correspondences_equal_the_oracles(world, name, n=None):
    """kicp_pass_correspondences - the EXPORT twin - query for query, and bit-equal to the latency-oriented build"""
    _, gmap, _ = world.scenes[name]
    f = world.frame(name, n)
    acc, onn, od, _, _, _ = world.want(name, n)
    idx, d2, nn = _reg(FOUR_WAVES).pass_correspondences(f, gmap, I, TAU)
    np.testing.assert_array_equal(idx >= 0, acc)
    np.testing.assert_array_equal(nn[acc], onn[acc])
    np.testing.assert_array_equal(np.sqrt(d2[acc]), od[acc])
    assert np.all(d2[~acc] == np.finfo(np.float64).max) and not nn[~acc].any()
    lidx, ld2, lnn = _reg(LATENCY).pass_correspondences(f, gmap, I, TAU)
    assert np.array_equal(idx, lidx) and np.array_equal(d2, ld2) and np.array_equal(nn, lnn)


def _single_call_equals_the_oracles(world, name, n=None):
    """one fused pass (the sums) and a whole registration through k_pass_gather32<256, 1, 4, false, false>"""
    _, gmap, _ = world.scenes[name]
    f = world.frame(name, n)
    acc, _, _, osums, opose, oit = world.want(name, n)
    reg, lat = _reg(FOUR_WAVES), _reg(LATENCY)
    sums = reg.pass_sums(f, gmap, I, TAU)
    assert sums[6] == osums[6] == acc.sum()
    np.testing.assert_allclose(sums[:6], osums[:6], rtol=1e-12, atol=1e-9)
    assert np.array_equal(sums, lat.pass_sums(f, gmap, I, TAU))
    pose = reg.ComputeRobotMotion(f, gmap, I, I, TAU)
    np.testing.assert_allclose(pose, opose, rtol=0, atol=POSE_TOL, equal_nan=True)
    assert reg.last_stats.iterations == oit
    assert np.array_equal(pose, lat.ComputeRobotMotion(f, gmap, I, I, TAU), equal_nan=True) and lat.last_stats.iterations == oit
    return pose


@pytest.mark.parametrize("name", CASES)
def test_correspondences_of_each_regime(world, name):
    _correspondences_equal_the_oracles(world, name)
    acc = world.want(name)[0]
    assert acc.any() and (name in ("halo", "across", "near", "deep")) == bool(acc.all())


@pytest.mark.parametrize("name", CASES)
def test_single_calls_of_each_regime(world, name):
    _single_call_equals_the_oracles(world, name)


@pytest.mark.parametrize("n", fc.LENGTHS)
def test_scans_that_end_inside_a_wave(world, n):
    """lanes without a query in the last wave and block; the scan's first points hold every own-voxel state and queries without an entry"""
    _correspondences_equal_the_oracles(world, "mixed", n)
    _single_call_equals_the_oracles(world, "mixed", n)


def test_a_scan_without_any_entry(world):
    """every lane's probe finds nothing (todo == 0 for the whole wave): no round at all, no correspondence"""
    scene, gmap, omap = world.scenes["mixed"]
    f = scene.frames["mixed"][scene.tags["mixed"] == "no_entry"]
    assert len(f) > 64 and not okicp.associate(omap, f, I, TAU)[0].any()
    for options in (FOUR_WAVES, LATENCY):
        idx, d2, nn = _reg(options).pass_correspondences(f, gmap, I, TAU)
        assert np.all(idx == -1) and np.all(d2 == np.finfo(np.float64).max) and not nn.any()
        assert _reg(options).pass_sums(f, gmap, I, TAU)[6] == 0


@pytest.mark.parametrize("which", ["cap20", "cap40"])
@pytest.mark.parametrize("T", TILES)
def test_batches_through_the_jobs_kernel(world, T, which):
    """eighteen scans - every regime, and the scans that end inside a wave - on the queues, four jobs per launch"""
    if which == "cap40":
        scans = [("deep", n) for n in (None, 700, 257, 1000, 65, 1199)] * 3
    else:
        scans = [(name, None) for name in ("halo", "across", "beyond", "near", "mixed")] + [("mixed", n) for n in fc.LENGTHS]
        scans = (scans + [("halo", 1100), ("beyond", 255), ("near", 65), ("across", 257)] + scans)[:18]
    _, gmap, _ = world.scenes[scans[0][0]]
    frames = [K.DeviceFrame(world.frame(name, n), device=0) for name, n in scans]
    reg = _reg(dict(GROUPED, batch_group=4, pass_tiles=T))
    b = reg.prepare_batch(frames, [I] * len(scans), [I] * len(scans))
    got = reg.ComputeRobotMotionBatch(b, gmap, TAU).copy()
    assert reg.get_option("batch_queue_passes") >= len(scans) and reg.get_option("batch_group_launches") > 0
    lat = _reg(LATENCY)
    for k, (name, n) in enumerate(scans):
        _, _, _, _, opose, oit = world.want(name, n)
        np.testing.assert_allclose(got[k], opose, rtol=0, atol=POSE_TOL, equal_nan=True, err_msg="%s %s" % (name, n))
        assert int(b.iterations[k]) == oit
        if k < 11:  # (every distinct scan once)
            assert np.array_equal(got[k], lat.ComputeRobotMotion(world.frame(name, n), gmap, I, I, TAU), equal_nan=True)
