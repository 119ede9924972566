"""Seeded operation-sequence fuzz of the voxel map (in the style of tests/test_gpu_fuzz.py): up to 8 operations - host AddPoints,
Update(points, origin), Update(points, pose), UpdateDevice, UpdateDeviceBegin finished or left for the next operation to collect,
RemovePointsFarFromLocation, Clear, copy() (going on with the copy, the original checked once more at the end), Pointcloud,
GetClosestNeighbor - on one K.VoxelHashMap and the oracle(s) in lock step, with plane / lattice / cluster point sets of 1 to 5 000
points (bulk insertions on device=0 maps) around a centre that walks a few voxels per operation, so that pruning and bucket re-use
happen.  Counts after every mutating operation; at the end the buckets point for point in order, check() == 0 and
GetClosestNeighbor bit for bit.  A module-level tally of update_counts() proves that the examples together ran both insertion
kernels, a device-side re-hash and a deferred update (120 examples, a second or two: hypothesis leans towards the first element of
every sampled_from in its early examples)."""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, seed, settings
from hypothesis import strategies as st

import kinematic_icp_amd as K
import mapdev_scenes as sc
from mapdev_ref import Oracles, assert_same_buckets, bucket_sorted

pytestmark = pytest.mark.gpu
OPS = ["add", "update_origin", "update_pose", "update_device", "update_device", "begin", "begin", "remove_far", "clear", "copy", "pointcloud",
       "closest"]
TALLY = dict(examples=0, apply_wave=0, apply_thread=0, rehashes=0, deferred=0, host_updates=0)


@st.composite
def programs(draw):
    vs = draw(st.sampled_from([0.25, 0.5, 1.0]))
    ops = []
    for _ in range(draw(st.integers(1, 8))):
        ops.append(dict(op=draw(st.sampled_from(OPS)), kind=draw(st.sampled_from(["plane", "lattice", "clusters"])),
                        n=draw(st.one_of(st.integers(1, 400), st.integers(1, 400), st.integers(400, 5000))),
                        extent=draw(st.sampled_from([3.0, 10.0])), walk=(draw(st.integers(-3, 3)), draw(st.integers(-3, 3))),
                        yaw=draw(st.sampled_from([0.0, 0.3, -2.0])), finish=draw(st.booleans())))
    return dict(seed=draw(st.integers(0, 2**32 - 1)), vs=vs, cap=draw(st.sampled_from([20, 256, 1, 3, 64, 255])),
                max_distance=draw(st.sampled_from([8.0 * vs, 30.0 * vs, 1e6])), device=draw(st.sampled_from([None, 0])), ops=ops)


def point_set(rng, kind, n, extent, vs):
    """n points around the origin, at most `extent` voxels out (far inside the +-2^20 voxels of the packed keys)"""
    e = extent * vs
    if kind == "plane":
        return np.concatenate([rng.uniform(-e, e, (n, 2)), rng.normal(0, 0.02 * vs, (n, 1))], 1)
    if kind == "lattice":  # multiples of vs / 8: points on voxel faces, exact ties, exact duplicates
        return np.round(rng.uniform(-e, e, (n, 3)) * np.array([1, 1, 0.2]) * 8 / vs) * vs / 8
    c = rng.uniform(-e, e, (max(1, n // 60), 3)) * np.array([1, 1, 0.2])
    return c[rng.integers(0, len(c), n)] + rng.normal(0, 0.3 * vs, (n, 3))


class CopyableOracles(Oracles):
    def clone(self, max_distance, cap):
        """the same map again: Pointcloud() lists every voxel's points in their order, and points that were accepted in that order are
        accepted in it again"""
        c = CopyableOracles(self.vs, max_distance, cap)
        c.AddPoints(self.o.Pointcloud())
        assert c.num_points() == self.num_points()
        return c


def same_counts(g, o, what):
    assert (g.num_points(), g.num_voxels()) == (o.num_points(), o.num_voxels()), what


@seed(20261018)
@settings(max_examples=120, deadline=None, suppress_health_check=list(HealthCheck), derandomize=True, database=None)
@given(programs())
def test_operation_sequences_against_the_oracle(pr):
    rng = np.random.default_rng(pr["seed"])
    vs, cap, md = pr["vs"], pr["cap"], pr["max_distance"]
    g, o = K.VoxelHashMap(vs, md, cap, device=pr["device"]), CopyableOracles(vs, md, cap)
    maps, frames, originals = [g], [], []
    centre = np.zeros(3)
    for k, op in enumerate(pr["ops"]):
        what = "operation %d: %s" % (k, op)
        centre = centre + np.array([op["walk"][0], op["walk"][1], 0.0]) * vs
        pose = np.concatenate([[0.0, 0.0, np.sin(0.5 * op["yaw"]), np.cos(0.5 * op["yaw"])], centre])
        local = point_set(rng, op["kind"], op["n"], op["extent"], vs)
        pending = False
        if op["op"] == "add":
            g.AddPoints(local + centre), o.AddPoints(local + centre)
        elif op["op"] == "update_origin":
            g.Update(local + centre, centre), o.Update(local + centre, centre)
        elif op["op"] == "update_pose":
            g.Update(local, pose), o.Update(local, pose)
        elif op["op"] in ("update_device", "begin"):
            frames.append(K.DeviceFrame(local))
            if op["op"] == "update_device":
                assert g.UpdateDevice(frames[-1], pose), what
            else:
                g.UpdateDeviceBegin(frames[-1], pose)
                if op["finish"]:
                    assert g.UpdateFinish(), what
                pending = not op["finish"]  # (left for the next operation on the map - or the final checks - to collect)
            o.Update(local, pose)
        elif op["op"] == "remove_far":
            g.RemovePointsFarFromLocation(centre), o.RemovePointsFarFromLocation(centre)
        elif op["op"] == "clear":
            g.Clear(), o.Clear()
            assert g.Empty()
        elif op["op"] == "copy":
            originals.append((g, o))
            g, o = g.copy(), o.clone(md, cap)
            maps.append(g)
        elif op["op"] == "pointcloud":
            np.testing.assert_array_equal(bucket_sorted(g.Pointcloud(), vs), o.buckets(), err_msg=what)
        else:
            q = local[:200] + centre
            (nn_g, d_g), (nn_o, d_o) = g.GetClosestNeighbor(q), o.GetClosestNeighbor(q)
            assert np.array_equal(d_g, d_o) and np.array_equal(nn_g, nn_o), what
        if not pending:
            same_counts(g, o, what)
    for gm, om in originals + [(g, o)]:
        same_counts(gm, om, "at the end")
        assert_same_buckets(gm, om, vs, "at the end")
        q = sc.jittered_queries(om.o.Pointcloud(), vs, n=300, seed=pr["seed"] % 1000) + (0 if om.num_points() else centre)
        (nn_g, d_g), (nn_o, d_o) = gm.GetClosestNeighbor(q), om.GetClosestNeighbor(q)
        assert np.array_equal(d_g, d_o) and np.array_equal(nn_g, nn_o)
    TALLY["examples"] += 1
    for m in maps:
        c = m.update_counts()
        for name in ("apply_wave", "apply_thread", "rehashes", "deferred", "host_updates"):
            TALLY[name] += c[name]


def test_the_sequences_entered_every_path():
    if TALLY["examples"] == 0:  # (selected on its own)
        test_operation_sequences_against_the_oracle()
    assert TALLY["apply_wave"] > 0 and TALLY["apply_thread"] > 0 and TALLY["rehashes"] > 0 and TALLY["deferred"] > 0, TALLY
    assert TALLY["host_updates"] == 0, TALLY  # no coordinate leaves the packed keys' range: nothing is handed to the host map
