"""The three single-GPU hand-offs of the generic pass kernel (kicp_pass_params.hpp: HandOff; kicp_pass_finish.hpp: finish_pass) give the same sums of pass 0,
as doubles, exactly:
  * group rows to the host: a registration of one iteration (stats.sums[0], stats.n_corr[0]);
  * totals left on the device, then k_publish_sums: kicp_pass_sums at the same pose;
  * totals left on the device, then the collective and k_publish_words: the same registration with an identity all-reduce attached.
The sums are exact integers whatever the path, and the host and k_publish_sums convert the limbs with the same operations.

One synthetic map of a few thousand points, option "small" 0 so that the generic kernel runs, two frame sizes - 300 points (two
workgroups at one lane per query, one group) and 33 * 256 + 5 = 8 453 points (34 workgroups, two groups: the totals take their
second reduction level, and the last block is partial) - each with one and with four lanes per query.

The pose: last_pose = identity and rel_odom = P with the unit quaternion (0, 0, 0.6, 0.8), whose norm is 1.0 exactly in fp64, so the
prediction last_pose * rel_odom the registration starts from is P bit for bit and kicp_pass_sums can be given the same pose."""
import numpy as np
import pytest

import kinematic_icp_amd as K

pytestmark = pytest.mark.gpu
VOXEL, TAU = 1.0, 0.8
IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
POSE = np.array([0.0, 0.0, 0.6, 0.8, 0.25, -0.125, 0.0])


@pytest.fixture(scope="module")
def world():
    rng = np.random.Generator(np.random.PCG64(20260))
    points = rng.uniform([-12.0, -12.0, 0.0], [12.0, 12.0, 2.0], size=(6000, 3))
    gmap = K.VoxelHashMap(VOXEL, 100.0, 20)
    gmap.AddPoints(points)
    frame = rng.uniform([-9.0, -9.0, 0.0], [9.0, 9.0, 2.0], size=(33 * 256 + 5, 3))
    return gmap, frame


def _reg(lanes):
    reg = K.KinematicRegistration(max_num_iteration=1)
    reg.set_option("small", 0)
    reg.set_option("lanes_per_query", lanes)
    return reg


def _first_pass(reg, frame, gmap):
    reg.ComputeRobotMotion(frame, gmap, IDENTITY, POSE, TAU)
    st = reg.last_stats
    assert st.iterations == 1
    return np.array(list(st.sums[0]) + [st.n_corr[0]])


@pytest.mark.parametrize("lanes", [1, 4])
@pytest.mark.parametrize("n", [300, 33 * 256 + 5])
def test_pass0_sums_equal_through_every_single_gpu_hand_off(world, n, lanes):
    gmap, frame = world
    frame = frame[:n]
    rows = _first_pass(_reg(lanes), frame, gmap)
    assert rows[6] > n / 8  # (a pass with correspondences)
    totals = _reg(lanes).pass_sums(frame, gmap, POSE, TAU)
    calls = []
    sharded = _reg(lanes)
    sharded.set_allreduce(lambda ptr, count, stream: calls.append(count))  # (world size 1: the sum in place is the buffer itself)
    words = _first_pass(sharded, frame, gmap)
    assert calls == [24]
    print("rows  ", rows.tolist(), "\ntotals", totals.tolist(), "\nwords ", words.tolist())
    assert np.array_equal(rows, totals) and np.array_equal(rows, words)
