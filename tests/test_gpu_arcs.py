"""A fan of arcs scored on the GPU (kicp_grid_score_arcs: K.OccupancyGrid.score_arcs) against the host entry
(K.score_arcs_from_plan) and the restatement of include/kicp.h's text (tests/arcs_ref.py).  Both sides execute the same IEEE
operations in the stated order, so everything is exact: np.array_equal, no tolerance anywhere.  The cases are the smallest shapes at
which the kernel's mapping - a wave per arc, four arcs per workgroup, lanes striding the samples - can go wrong."""
import ctypes as C

import numpy as np
import pytest

import kinematic_icp_amd as K
import arcs_ref as ar
import clearance_ref as cr
import potential_ref as pr
from test_arcs_host import check_case

pytestmark = pytest.mark.gpu

CASES = ar.small_cases()


def grid_for(q, cell, origin_x, origin_y):
    return K.OccupancyGrid(cell, origin_x, origin_y, q.shape[1], q.shape[0], 0.0, 1.0, 1.0)


def check(grid, q, pot, cell, ox, oy, start, arcs, n_steps, footprint):
    """the device against the host entry and the restatement; -> the results"""
    got = grid.score_arcs(start, arcs, n_steps, footprint)
    assert got.dtype == np.uint32 and got.shape == (len(arcs), 4)
    host = K.score_arcs_from_plan(q, pot, cell, ox, oy, start, arcs, n_steps, footprint)
    want = ar.score_arcs(q, pot, cell, ox, oy, start, arcs, n_steps, footprint)
    bad = (got != want).any(axis=1)
    print("%d x %d, %d arcs of %d steps, %d samples: %d arcs differ; free steps min %d max %d, %d end early" %
          (q.shape[1], q.shape[0], len(arcs), n_steps, len(footprint), bad.sum(), want[:, 0].min(), want[:, 0].max(), (want[:, 0] < n_steps).sum()))
    assert np.array_equal(host, want)
    assert not bad.any(), (np.flatnonzero(bad)[:5], got[bad][:5], want[bad][:5])
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_small_cases(name):
    """P = 1, 63, 64, 65, 130; K = 1, 3, 4, 5, 257; T = 1; arcs that collide at step 1, at step T and never; grids of 1 x 1 and 33 x 31;
    arcs leaving over each of the four sides; a start outside the grid; a spin in place; NaN and +-inf in an arc's row and in a
    footprint sample; a sample whose quotient is an exact integer; an end cell that is unreached and one at the clamp; the fuzz of 2 000
    random arcs of 24 steps on 70 x 50 cells with 30 % impassable under a 5 x 3 box, and one on a sparser map where arcs run long"""
    q, goals, max_potential, cell, ox, oy, start, arcs, n_steps, footprint = CASES[name]
    grid = grid_for(q, cell, ox, oy)
    pot = grid.potential_of_costmap(q, pr.IDENTITY, goals, max_potential)
    got = check(grid, q, pot, cell, ox, oy, start, arcs, n_steps, footprint)
    check_case(name, got, n_steps, pot)


def test_three_calls_on_one_handle_with_k_growing_and_shrinking():
    """4 -> 257 -> 4 arcs: the buffers grow between calls, and the third call must not read what the second left"""
    q, goals, max_potential, cell, ox, oy, start, arcs, n_steps, footprint = CASES["arcs_257"]
    grid = grid_for(q, cell, ox, oy)
    pot = grid.potential_of_costmap(q, pr.IDENTITY, goals, max_potential)
    first = check(grid, q, pot, cell, ox, oy, start, arcs[:4], n_steps, footprint)
    second = check(grid, q, pot, cell, ox, oy, start, arcs, n_steps, footprint)
    third = check(grid, q, pot, cell, ox, oy, start, arcs[253:], n_steps, footprint[:7])
    assert np.array_equal(first, second[:4]) and third.shape == (4, 4)
    out = np.zeros((4, 4), dtype=np.uint32)
    assert grid.score_arcs(start, arcs[:4], n_steps, footprint, out=out) is out and np.array_equal(out, first)  # written in place


def test_plan_validity():
    """no plan before a potential call; kicp_grid_costmap and integrating a frame in between change nothing; a second potential call
    with other goals gives the new plan; a potential call that fails leaves none"""
    occ = cr.random_occupancy(90, 60, 0.01, 31, unknown_fraction=0.03)
    occ[20:40, 30:60] = 0
    grid = K.OccupancyGrid(0.05, -1.0, -0.5, 90, 60, 0.0, 1.0, 1.0)
    grid.set_counts(cr.counts_of(occ))
    table, weight = K.nav2_cost_table(0.05, 3, 0.05, 3.0), K.plan_weights(unknown_weight=200)
    rng = np.random.Generator(np.random.PCG64(8))
    arcs, footprint = ar.random_arcs(rng, 40, step=0.08), ar.footprint_box(-0.06, 0.06, -0.04, 0.04, 0.04)
    start = ar.centre(0.05, -1.0, -0.5, 45, 30) + (1.0, 0.0)

    def code(fn, *a, **kw):
        with pytest.raises(K.KicpError) as e:
            fn(*a, **kw)
        return e.value.code, str(e.value)

    assert not grid.has_plan()
    c, msg = code(grid.score_arcs, start, arcs, 10, footprint)
    assert c == K.KICP_ERR_ARG and "kicp_grid_potential" in msg
    grid.costmap(table)  # neither a costmap nor a clearance makes a plan
    grid.clearance(3)
    assert not grid.has_plan() and code(grid.score_arcs, start, arcs, 10, footprint)[0] == K.KICP_ERR_ARG

    pot = grid.potential(table, weight, [(45, 30)])
    costmap = grid.costmap(table)  # after the plan was made: writes none of its buffers
    assert grid.has_plan()
    q = K.plan_q(costmap, weight)
    first = check(grid, q, pot, 0.05, -1.0, -0.5, start, arcs, 10, footprint)
    assert (first[:, 0] == 10).any() and (first[:, 3] != ar.UNREACHED).any()
    grid.clearance(3)
    grid.costmap(table, inflate_unknown=True, rect=(3, 4, 20, 10))
    assert np.array_equal(grid.score_arcs(start, arcs, 10, footprint), first)
    # a frame changes the counters, not the plan: the plan is a snapshot
    grid.integrate(np.array([[0.5, 0.0, 0.5], [0.3, 0.2, 0.5]]), np.array([0.0, 0.0, 0.0, 1.0, 1.25, 1.0, 0.0]))
    assert grid.has_plan() and np.array_equal(grid.score_arcs(start, arcs, 10, footprint), first)
    grid.set_counts(cr.counts_of(occ))

    pot2 = grid.potential(table, weight, [(5, 5), (80, 50)])
    assert not np.array_equal(pot2, pot)
    second = check(grid, q, pot2, 0.05, -1.0, -0.5, start, arcs, 10, footprint)
    assert np.array_equal(second[:, :3], first[:, :3]) and not np.array_equal(second[:, 3], first[:, 3])  # the same q, the new potential
    other = pr.random_costmap(90, 60, 3, 0.05)
    pot3 = grid.potential_of_costmap(other, pr.IDENTITY, [(45, 30)], 5000)
    check(grid, other, pot3, 0.05, -1.0, -0.5, start, arcs, 10, footprint)

    assert code(grid.potential_of_costmap, other, pr.IDENTITY, [(90, 0)])[0] == K.KICP_ERR_ARG  # a goal outside the grid
    assert not grid.has_plan() and code(grid.score_arcs, start, arcs, 10, footprint)[0] == K.KICP_ERR_ARG
    grid.potential_of_costmap(other, pr.IDENTITY, [(45, 30)], 5000)
    assert code(grid.potential, table, weight, [(45, 30)], min_observations=0)[0] == K.KICP_ERR_ARG  # the library's own refusal, on an argument
    assert not grid.has_plan()
    pot4 = grid.potential_of_costmap(other, pr.IDENTITY, [(45, 30)], 5000)
    assert grid.has_plan() and np.array_equal(pot4, pot3)
    check(grid, other, pot4, 0.05, -1.0, -0.5, start, arcs, 10, footprint)


def test_argument_errors_on_the_device():
    q, potential, cell, start, arcs, n_steps, footprint, want = ar.pinned_8x6()
    grid = grid_for(q, cell, 0.0, 0.0)
    pot = grid.potential_of_costmap(q, pr.IDENTITY, [(0, 0)])
    got = grid.score_arcs(start, arcs, n_steps, footprint)
    assert np.array_equal(got[:, :3], want[:, :3]) and got[:, 3].tolist() == [int(pot[1, 3]), int(pot[1, 1])]  # the pinned case, with the field's own potential

    def code(**kw):
        with pytest.raises(K.KicpError) as e:
            grid.score_arcs(**{**dict(start=start, arcs=arcs, n_steps=n_steps, footprint=footprint), **kw})
        return e.value.code, str(e.value)

    for kw in (dict(n_steps=0), dict(n_steps=-1), dict(arcs=np.zeros((0, 4))), dict(footprint=np.zeros((0, 2))), dict(start=(0.75, 0.75, float("nan"), 0.0)),
               dict(start=(0.75, float("-inf"), 1.0, 0.0)), dict(start=(0.75, 0.75, 1.0)), dict(arcs=np.zeros((2, 3))), dict(footprint=np.zeros((3, 3))),
               dict(out=np.zeros((2, 4), dtype=np.int32)), dict(out=np.zeros((3, 4), dtype=np.uint32))):
        assert code(**kw)[0] == K.KICP_ERR_ARG, kw
    for kw, limit in ((dict(n_steps=1025), "1024"), (dict(footprint=np.zeros((4097, 2))), "4096"), (dict(arcs=np.zeros(((1 << 20) + 1, 4))), str(1 << 20))):
        c, msg = code(**kw)
        assert c == K.KICP_ERR_CAPACITY and limit in msg, (kw, msg)

    lib = K.lib()
    dp, u32 = C.POINTER(C.c_double), C.POINTER(C.c_uint)
    s, a, f = np.array(start), np.ascontiguousarray(arcs), np.ascontiguousarray(footprint)
    res = np.zeros(8, dtype=np.uint32)
    good = [grid._h, s.ctypes.data_as(dp), a.ctypes.data_as(dp), 2, 4, f.ctypes.data_as(dp), 3, res.ctypes.data_as(u32), 8]
    assert lib.kicp_grid_score_arcs(*good) == K.KICP_OK and np.array_equal(res.reshape(2, 4), got)
    for k, v in ((0, None), (1, None), (2, None), (5, None), (7, None), (3, 0), (4, 0), (6, 0), (8, 7), (8, 9)):
        bad = list(good)
        bad[k] = v
        assert lib.kicp_grid_score_arcs(*bad) == K.KICP_ERR_ARG, k
    assert lib.kicp_grid_has_plan(None) == 0 and lib.kicp_grid_has_plan(grid._h) == 1
    assert np.array_equal(grid.score_arcs(start, arcs, n_steps, footprint), got)  # the handle and its plan are unharmed
    # the limits themselves are legal: 1 024 steps, and 4 096 samples that all lie on the base's origin
    assert grid.score_arcs(start, arcs[1:], 1024, footprint).tolist() == [[1024, 10 + 20 * 1023 - 10 * 255, 20, int(pot[1, 1])]]
    assert np.array_equal(grid.score_arcs(start, arcs, n_steps, np.zeros((4096, 2)))[:, 0], K.score_arcs_from_plan(q, pot, cell, 0.0, 0.0, start, arcs, n_steps, np.zeros((4096, 2)))[:, 0])
