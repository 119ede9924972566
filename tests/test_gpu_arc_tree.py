"""A tree of arc segments scored on the GPU (kicp_grid_score_arc_tree: K.OccupancyGrid.score_arc_tree) against the host entry
(K.score_arc_tree_from_plan) and the restatement of include/kicp.h's text (tests/arc_tree_ref.py), which rolls every node from the
start on its own: equality also shows that continuing the records of the level above changes no bit.  All sides execute the same
IEEE operations in the stated order, so everything is exact: np.array_equal, no tolerance anywhere.  The cases are the smallest shapes
at which the kernel's mapping - a launch per level, a wave per node, four nodes per workgroup, the parent and the primitive by
division, lanes striding the samples - can go wrong."""
import ctypes as C

import numpy as np
import pytest

import kinematic_icp_amd as K
import arcs_ref as ar
import arc_tree_ref as tr
import clearance_ref as cr
import potential_ref as pr

pytestmark = pytest.mark.gpu

CASES = tr.small_cases()


def grid_for(q, cell, origin_x, origin_y):
    return K.OccupancyGrid(cell, origin_x, origin_y, q.shape[1], q.shape[0], 0.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def reference():
    """name -> (potential, rows by the restatement, the nodes' classes) on the host's field - computed once"""
    out = {}
    for name, case in CASES.items():
        q, goals, max_potential = case[:3]
        pot = K.potential_from_costmap(q, pr.IDENTITY, goals, max_potential)
        out[name] = (pot,) + tr.score_tree(q, pot, *case[3:], return_classes=True)
    return out


def check(grid, q, pot, cell, ox, oy, start, branch, steps, primitives, footprint, want=None):
    """the device against the host entry and the restatement; -> the results"""
    got = grid.score_arc_tree(start, branch, steps, primitives, footprint)
    n_nodes, n_leaves, total, offsets = K.arc_tree_nodes(branch, steps)
    assert got.dtype == np.uint32 and got.shape == (n_nodes, 4)
    host = K.score_arc_tree_from_plan(q, pot, cell, ox, oy, start, branch, steps, primitives, footprint)
    if want is None:
        want = tr.score_tree(q, pot, cell, ox, oy, start, branch, steps, primitives, footprint)
    bad = (got != want).any(axis=1)
    print("%d x %d, branch %s steps %s, %d nodes, %d samples: %d nodes differ; free steps min %d max %d of %d" %
          (q.shape[1], q.shape[0], tuple(branch), tuple(steps), n_nodes, len(footprint), bad.sum(), want[:, 0].min(), want[:, 0].max(), total))
    assert np.array_equal(host, want)
    assert not bad.any(), (np.flatnonzero(bad)[:5], got[bad][:5], want[bad][:5])
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_small_cases(name, reference):
    """1, 3, 4, 5 and 257 nodes at the last level of a tree of depth 2 and at the only level of one of depth 1 (there against
    grid.score_arcs too); 1, 63, 64, 65 and 130 samples; steps (1, 1); depth 8; the wall with parents that collide at their first step,
    at their last and never, and a child that collides at its own first step; NaN and +-inf in a level-2 row and in a sample; a start
    outside the grid; paths over each side; an end cell that is unreached and one at the clamp; the fuzz of branch (8, 6, 5)"""
    q, goals, max_potential, cell, ox, oy, start, branch, steps, primitives, footprint = CASES[name]
    pot, want, classes = reference[name]
    grid = grid_for(q, cell, ox, oy)
    assert np.array_equal(grid.potential_of_costmap(q, pr.IDENTITY, goals, max_potential), pot)
    got = check(grid, q, pot, cell, ox, oy, start, branch, steps, primitives, footprint, want)
    tr.check_case(name, got, classes, branch, steps, pot)
    if len(branch) == 1:
        assert np.array_equal(grid.score_arcs(start, primitives, steps[0], footprint), got)
    if name == "fuzz_8_6_5":  # the three ways a node below level 1 can end are all well represented: the case cannot go vacuous
        below = np.bincount(classes[branch[0]:], minlength=3)
        print("below level 1: inherited %d, ended in their own segment %d, alive %d of %d" % (below[tr.INHERITED], below[tr.OWN], below[tr.ALIVE], below.sum()))
        assert below.sum() == 48 + 240 and (10 * below >= below.sum()).all()


def test_three_calls_on_one_handle_growing_and_shrinking():
    """a small tree, the fuzz's, then a small one with fewer samples: the buffers grow between calls, and the third call must not read
    what the second left - records included"""
    q, goals, max_potential, cell, ox, oy, start, branch, steps, primitives, footprint = CASES["fuzz_8_6_5"]
    grid = grid_for(q, cell, ox, oy)
    pot = grid.potential_of_costmap(q, pr.IDENTITY, goals, max_potential)
    small = primitives[[0, 1, 8, 9, 14]]
    first = check(grid, q, pot, cell, ox, oy, start, (2, 2, 1), (5, 4, 3), small, footprint)
    second = check(grid, q, pot, cell, ox, oy, start, branch, steps, primitives, footprint)
    third = check(grid, q, pot, cell, ox, oy, start, (2, 2, 1), (5, 4, 3), primitives[[3, 2, 9, 8, 15]], footprint[:7])
    assert np.array_equal(first[:2], second[:2]) and np.array_equal(first[2:4], second[8:10]) and third.shape == (10, 4)
    out = np.zeros((10, 4), dtype=np.uint32)
    assert grid.score_arc_tree(start, (2, 2, 1), (5, 4, 3), small, footprint, out=out) is out and np.array_equal(out, first)  # written in place


def test_plan_validity():
    """no plan before a potential call, with kicp_grid_score_arcs' message; kicp_grid_costmap, kicp_grid_clearance and integrating a
    frame in between change nothing; a potential call that fails leaves none"""
    occ = cr.random_occupancy(90, 60, 0.01, 31, unknown_fraction=0.03)
    occ[20:40, 30:60] = 0
    grid = K.OccupancyGrid(0.05, -1.0, -0.5, 90, 60, 0.0, 1.0, 1.0)
    grid.set_counts(cr.counts_of(occ))
    table, weight = K.nav2_cost_table(0.05, 3, 0.05, 3.0), K.plan_weights(unknown_weight=200)
    rng = np.random.Generator(np.random.PCG64(8))
    branch, steps = (5, 4), (6, 4)
    primitives, footprint = ar.random_arcs(rng, 9, step=0.08), ar.footprint_box(-0.06, 0.06, -0.04, 0.04, 0.04)
    start = ar.centre(0.05, -1.0, -0.5, 45, 30) + (1.0, 0.0)

    def code(fn, *a, **kw):
        with pytest.raises(K.KicpError) as e:
            fn(*a, **kw)
        return e.value.code, str(e.value)

    assert not grid.has_plan()
    c, msg = code(grid.score_arc_tree, start, branch, steps, primitives, footprint)
    assert c == K.KICP_ERR_ARG and msg == code(grid.score_arcs, start, primitives, 10, footprint)[1] and "kicp_grid_potential" in msg
    grid.costmap(table)  # neither a costmap nor a clearance makes a plan
    grid.clearance(3)
    assert code(grid.score_arc_tree, start, branch, steps, primitives, footprint)[0] == K.KICP_ERR_ARG

    pot = grid.potential(table, weight, [(45, 30)])
    q = K.plan_q(grid.costmap(table), weight)
    first = check(grid, q, pot, 0.05, -1.0, -0.5, start, branch, steps, primitives, footprint)
    assert (first[:, 0] > 0).any() and (first[:, 3] != ar.UNREACHED).any()
    grid.clearance(3)
    grid.costmap(table, inflate_unknown=True, rect=(3, 4, 20, 10))
    assert np.array_equal(grid.score_arc_tree(start, branch, steps, primitives, footprint), first)
    grid.integrate(np.array([[0.5, 0.0, 0.5], [0.3, 0.2, 0.5]]), np.array([0.0, 0.0, 0.0, 1.0, 1.25, 1.0, 0.0]))  # the plan is a snapshot
    assert grid.has_plan() and np.array_equal(grid.score_arc_tree(start, branch, steps, primitives, footprint), first)

    other = pr.random_costmap(90, 60, 3, 0.05)
    assert code(grid.potential_of_costmap, other, pr.IDENTITY, [(90, 0)])[0] == K.KICP_ERR_ARG  # a goal outside the grid
    assert not grid.has_plan() and code(grid.score_arc_tree, start, branch, steps, primitives, footprint)[0] == K.KICP_ERR_ARG
    pot2 = grid.potential_of_costmap(other, pr.IDENTITY, [(45, 30)], 5000)
    check(grid, other, pot2, 0.05, -1.0, -0.5, start, branch, steps, primitives, footprint)


def test_argument_errors_on_the_device():
    q, potential, cell, start, _, _, footprint, _ = ar.pinned_8x6()
    branch, steps, primitives, want = tr.pinned_8x6_tree()
    grid = grid_for(q, cell, 0.0, 0.0)
    pot = grid.potential_of_costmap(q, pr.IDENTITY, [(0, 0)])
    got = grid.score_arc_tree(start, branch, steps, primitives, footprint)
    ends = [(2, 1), (2, 1), (3, 1), (3, 2), (2, 3), (1, 2)]  # the pinned case, with the field's own potential
    assert np.array_equal(got[:, :3], want[:, :3]) and got[:, 3].tolist() == [int(pot[y, x]) for x, y in ends]

    def code(**kw):
        with pytest.raises(K.KicpError) as e:
            grid.score_arc_tree(**{**dict(start=start, branch=branch, steps=steps, primitives=primitives, footprint=footprint), **kw})
        return e.value.code, str(e.value)

    for kw in (dict(branch=(), steps=()), dict(branch=(2, 0)), dict(steps=(0, 2)), dict(steps=(1,)), dict(primitives=primitives[:3]), dict(primitives=np.zeros((4, 3))),
               dict(footprint=np.zeros((0, 2))), dict(footprint=np.zeros((3, 3))), dict(start=(0.75, 0.75, float("nan"), 0.0)), dict(start=(0.75, float("-inf"), 1.0, 0.0)),
               dict(start=(0.75, 0.75, 1.0)), dict(out=np.zeros((6, 4), dtype=np.int32)), dict(out=np.zeros((4, 4), dtype=np.uint32))):
        assert code(**kw)[0] == K.KICP_ERR_ARG, kw
    for kw, limit in ((dict(steps=(1000, 25)), "1024"), (dict(footprint=np.zeros((4097, 2))), "4096"), (dict(branch=(1024, 1024), primitives=np.zeros((2048, 4))), str(1 << 20)),
                      (dict(branch=(1,) * 9, steps=(1,) * 9, primitives=np.zeros((9, 4))), "8")):
        c, msg = code(**kw)
        assert c == K.KICP_ERR_CAPACITY and limit in msg, (kw, msg)

    lib = K.lib()
    dp, u32 = C.POINTER(C.c_double), C.POINTER(C.c_uint)
    s, p, f = np.array(start), np.ascontiguousarray(primitives), np.ascontiguousarray(footprint)
    b, st = np.array(branch, dtype=np.uint32), np.array(steps, dtype=np.uint32)
    res = np.zeros(24, dtype=np.uint32)
    good = [grid._h, s.ctypes.data_as(dp), 2, b.ctypes.data_as(u32), st.ctypes.data_as(u32), p.ctypes.data_as(dp), f.ctypes.data_as(dp), 3, res.ctypes.data_as(u32), 24]
    assert lib.kicp_grid_score_arc_tree(*good) == K.KICP_OK and np.array_equal(res.reshape(6, 4), got)
    for k, v in ((0, None), (1, None), (3, None), (4, None), (5, None), (6, None), (8, None), (2, 0), (7, 0), (9, 23), (9, 25), (9, 16)):
        bad = list(good)
        bad[k] = v
        assert lib.kicp_grid_score_arc_tree(*bad) == K.KICP_ERR_ARG, k
    for k, v in ((2, 9), (7, 4097)):
        bad = list(good)
        bad[k] = v
        assert lib.kicp_grid_score_arc_tree(*bad) == K.KICP_ERR_CAPACITY, k
    assert np.array_equal(grid.score_arc_tree(start, branch, steps, primitives, footprint), got)  # the handle and its plan are unharmed
    # the limits themselves are legal: 1 024 steps along a path - the quarter turns circle four cells - and 4 096 samples on the base's origin
    assert np.array_equal(grid.score_arc_tree(start, (2, 1), (1, 1023), primitives[[0, 1, 3]], footprint), K.score_arc_tree_from_plan(q, pot, cell, 0.0, 0.0, start, (2, 1), (1, 1023), primitives[[0, 1, 3]], footprint))
    assert grid.score_arc_tree(start, (2, 1), (1, 1023), primitives[[0, 1, 3]], footprint)[3, 0] == 1024
    many = np.zeros((4096, 2))
    assert np.array_equal(grid.score_arc_tree(start, branch, steps, primitives, many), K.score_arc_tree_from_plan(q, pot, cell, 0.0, 0.0, start, branch, steps, primitives, many))


def test_a_tree_of_2_to_the_20_nodes():
    """branch (1024, 1023) is exactly 2^20 nodes: 262 144 workgroups at the last level under 1 024 records; one step a level and one
    sample.  The device against the host entry only"""
    q = pr.random_costmap(70, 50, 12, 0.1)
    rng = np.random.Generator(np.random.PCG64(21))
    start, at = ar.open_start(q, 0.25, -1.0, -2.0, rng)
    grid = grid_for(q, 0.25, -1.0, -2.0)
    pot = grid.potential_of_costmap(q, pr.IDENTITY, [at])
    branch, steps = (1024, 1023), (1, 1)
    primitives, footprint = ar.random_arcs(rng, 2047, step=1.5, turn=1.0), np.array([[0.05, 0.0]])
    got = grid.score_arc_tree(start, branch, steps, primitives, footprint)
    host = K.score_arc_tree_from_plan(q, pot, 0.25, -1.0, -2.0, start, branch, steps, primitives, footprint)
    assert got.shape == (1 << 20, 4) and np.array_equal(got, host)
    free = np.bincount(got[1024:, 0], minlength=3)
    print("the leaves' free steps 0 / 1 / 2:", free.tolist())
    assert (free > 1000).all()  # inherited from a parent that collided, ended at their own step, alive
    leaf, path = K.arc_tree_best(got, branch, steps)
    assert got[1024 + leaf, 3] == got[1024:][got[1024:, 0] >= 1, 3].min() and leaf == path[0] * 1023 + path[1]
