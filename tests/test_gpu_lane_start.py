"""The start of a lane and the set-up of a visit (kicp_pass_visit.hpp: voxel_coord's constant guard, the lane offsets taken from its
fraction, query_from for each of the 27 shifts, the lending round's integer minima) through every build of the pass kernel a handle can
pick, on the scenes of tests/lane_start_cases.py, whose premises() proves on the CPU that each regime is entered: a query whose accepted
neighbour lies in each of the 27 shifts, coordinates exactly on voxel faces, coordinates inside the constant guard but outside the one
it replaced (both sides, every axis), coordinates where the reciprocal's floor is not the division's, negative coordinates, waves whose
loaded lanes lend two voxels each from round 2, scans of 1, 255, 256, 257 and 512 queries.

Every build is held to the oracle bit for bit (np.array_equal): the correspondences query for query through kicp_pass_correspondences
(the same queries accepted, the same map point, the same distance), the pose and the number of iterations of a registration from the
identity - the scenes are built so that the sums of J^T r are exact and 0, lane_start_cases.py says how.  A batch of scans through the
job list's kernel returns the oracle's bits as well.  The builds are those of tests/test_gpu_mirror_z.py; the oracle's results of a scene
are computed once."""
import numpy as np
import pytest

import kinematic_icp_amd as K
import lane_start_cases as lc
import test_gpu_mirror_z as mz
from checkers import okicp

pytestmark = pytest.mark.gpu
I = lc.I
SCENES = sorted(lc.BUILDERS)
BUILD_NAMES = [name for name, _ in mz.BUILDS]


class World:
    """the scenes, their maps and the oracle's answers - computed once, never changed"""

    def __init__(self):
        self.scenes = {}
        for name in SCENES:
            scene = lc.BUILDERS[name]()
            omap = lc.oracle_map(scene)
            lc.premises(scene, omap)
            gmap = K.VoxelHashMap(scene.vs, 100.0, scene.cap)
            gmap.AddPoints(scene.map_points)
            assert gmap.num_points() == len(scene.map_points) and gmap.check() == 0
            acc, nn, d = okicp.associate(omap, scene.queries, I, scene.tau)
            oreg = okicp.KinematicRegistration()
            pose = oreg.ComputeRobotMotion(scene.queries, omap, I, I, scene.tau)
            self.scenes[name] = (scene, gmap, (acc, nn, d, pose, oreg.last_stats.iterations))


@pytest.fixture(scope="module")
def world():
    return World()


def _named(scene, rows):
    return sorted(set(scene.tags[rows]))


@pytest.mark.parametrize("build", BUILD_NAMES)
@pytest.mark.parametrize("name", SCENES)
def test_every_build_equals_the_oracle(world, name, build):
    scene, gmap, (acc, onn, od, opose, oit) = world.scenes[name]
    reg = mz._reg(dict(mz.BUILDS)[build])
    idx, d2, nn = reg.pass_correspondences(scene.queries, gmap, I, scene.tau)
    wrong = np.flatnonzero(((idx >= 0) != acc) | np.any(nn != np.where(acc[:, None], onn, 0.0), axis=1))
    assert len(wrong) == 0, _named(scene, wrong)  # (names the cases: "shift_13", "guard_2_low", "tenth_up" ...)
    assert np.array_equal(idx >= 0, acc) and np.array_equal(nn[acc], onn[acc]) and np.array_equal(np.sqrt(d2[acc]), od[acc])
    assert np.all(idx[~acc] == -1) and np.all(d2[~acc] == np.finfo(np.float64).max)
    pose = reg.ComputeRobotMotion(scene.queries, gmap, I, I, scene.tau)
    assert np.array_equal(pose, opose), (pose, opose)
    assert reg.last_stats.iterations == oit == 1


def test_a_batch_through_the_job_list_equals_the_oracle(world):
    """every scene goes through a batch of its own, eighteen times its scan (a part of a scan would break the pairs that keep J^T r at
    0): two lanes need two groups of four jobs each before the job list's kernel runs"""
    for name in SCENES:
        scene, gmap, (_, _, _, opose, oit) = world.scenes[name]
        scans = [scene.queries] * 18
        frames = [K.DeviceFrame(s, device=0) for s in scans]
        reg = mz._reg(mz.GROUPED)
        b = reg.prepare_batch(frames, [I] * len(scans), [I] * len(scans))
        got = reg.ComputeRobotMotionBatch(b, gmap, scene.tau).copy()
        assert reg.get_option("batch_group_launches") > 0
        for k in range(len(scans)):
            assert np.array_equal(got[k], opose), (name, k, got[k])
            assert int(b.iterations[k]) == oit
