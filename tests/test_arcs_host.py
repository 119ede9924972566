"""Scoring a fan of arcs without a GPU: the pure-host entries (K.score_arcs_from_plan, K.plan_q, K.arc_steps, K.footprint_box,
K.arcs_best) against the restatement of include/kicp.h's text in Python floats (tests/arcs_ref.py) - np.array_equal, no tolerance - a
pinned 8 x 6 case with its numbers written out, the argument and capacity errors, and the shared header (kicp_arcs_host.hpp: the very
arithmetic the kernel calls) in a stand-alone program, built plainly and under ASan + UBSan, on the same cases."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
import arcs_ref as ar
import potential_ref as pr

CASES = ar.small_cases()


def plan_of(case):
    """(q, potential) of a case, on the host"""
    q, goals, max_potential = case[:3]
    return q, K.potential_from_costmap(q, pr.IDENTITY, goals, max_potential)


@pytest.fixture(scope="module")
def reference():
    """name -> (potential, results by the restatement) - computed once"""
    out = {}
    for name, case in CASES.items():
        q, pot = plan_of(case)
        out[name] = pot, ar.score_arcs(q, pot, *case[3:])
    return out


def test_arc_steps_equal_the_restatement_bit_for_bit():
    """first of all: math.sin / math.cos and the library's host code call the same libm, so the arcs are equal bit for bit"""
    rng = np.random.Generator(np.random.PCG64(1))
    v, omega = rng.uniform(-2.0, 2.0, 20000), rng.uniform(-3.0, 3.0, 20000)
    omega[:12] = [0.0, -0.0, 1e-9, -1e-9, 1e-10, -1e-10, 9.999e-10, 1e-9 * (1 + 1e-15), 5e-10, 1e-300, math.pi, -math.pi]
    for dt in (0.1, 1.0, 0.37):
        got, want = K.arc_steps(v, omega, dt), ar.arc_steps(v, omega, dt)
        assert got.dtype == np.float64 and got.shape == (20000, 4)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.abs(got - want).max()
    # below the threshold the arc is the straight line: where the reference's theta + epsilon would divide by zero nothing is divided
    eps = K.arc_steps([1.0, 1.0, 2.0], [-1e-10, 0.0, 5e-10], 1.0)
    assert np.array_equal(eps[:, :2], [[1.0, 0.0], [1.0, 0.0], [2.0, 0.0]]) and np.array_equal(eps[:, 2], np.cos([-1e-10, 0.0, 5e-10]))
    quarter = K.arc_steps([math.pi / 2], [math.pi / 2], 1.0)[0]  # a quarter circle of radius 1 ends at (1, 1), heading +y
    assert abs(quarter[0] - 1.0) < 1e-15 and abs(quarter[1] - 1.0) < 1e-15 and abs(quarter[2]) < 1e-16 and quarter[3] == 1.0
    out = np.zeros((3, 4))
    assert K.arc_steps([1.0, 1.0, 2.0], [-1e-10, 0.0, 5e-10], 1.0, out=out) is out and np.array_equal(out, eps)
    nan = K.arc_steps([1.0], [float("nan")], 1.0)
    assert np.isnan(nan).all()  # legal input: such an arc collides


def test_pinned_8x6_case():
    q, potential, cell, start, arcs, n_steps, footprint, want = ar.pinned_8x6()
    assert np.array_equal(ar.score_arcs(q, potential, cell, 0.0, 0.0, start, arcs, n_steps, footprint), want)
    got = K.score_arcs_from_plan(q, potential, cell, 0.0, 0.0, start, arcs, n_steps, footprint)
    assert got.dtype == np.uint32 and got.shape == (2, 4) and np.array_equal(got, want)
    assert want.tolist() == [[2, 60, 50, 103], [4, 70, 20, 101]]
    # one step fewer: the straight arc is unchanged, the turning one loses its last pose
    assert K.score_arcs_from_plan(q, potential, cell, 0.0, 0.0, start, arcs, 3, footprint).tolist() == [[2, 60, 50, 103], [3, 50, 20, 201]]
    assert K.arcs_best(want, n_steps) == 1 and K.arcs_best(want, n_steps, w_potential=0, w_cost=1) == 0
    assert np.array_equal(K.plan_q(np.array([[0, 1, 252], [253, 254, 255]], dtype=np.uint8), K.plan_weights()), [[50, 50, 251], [0, 0, 0]])


@pytest.mark.parametrize("name", sorted(CASES))
def test_score_arcs_from_plan(name, reference):
    q, goals, max_potential, cell, ox, oy, start, arcs, n_steps, footprint = CASES[name]
    pot, want = reference[name]
    assert np.array_equal(K.plan_q(q, pr.IDENTITY), q)
    got = K.score_arcs_from_plan(q, pot, cell, ox, oy, start, arcs, n_steps, footprint)
    assert got.dtype == np.uint32 and got.shape == (len(arcs), 4) and np.array_equal(got, want), np.argwhere(got != want)[:5]
    check_case(name, want, n_steps, pot)
    free, total, largest = want[:, 0].astype(int), want[:, 1].astype(int), want[:, 2].astype(int)
    assert (free <= n_steps).all() and (largest * free >= total).all() and (total >= largest).all() and ((free == 0) == (largest == 0)).all()


def check_case(name, res, n_steps, pot):
    """what each case is there for shows in its result (shared with the GPU suite)"""
    free = res[:, 0].tolist()
    if name == "wall_steps_5":
        assert free == [0, n_steps - 1, n_steps] and res[0].tolist() == [0, 0, 0, int(pot[15, 10])]  # at step 1, at step T, never
    if name == "wall_steps_1":
        assert free == [0, 1, 1]
    if name == "grid_1x1":
        assert res.tolist() == [[3, 27, 9, 0], [1, 9, 9, 0], [1, 9, 9, 0], [3, 27, 9, 0]]
    if name == "four_sides":
        assert all(0 < f < n_steps for f in free) and (res[:, 3] != ar.UNREACHED).all()
    if name == "start_outside":
        assert res[0].tolist() == [0, 0, 0, ar.UNREACHED] and free[1] == 3
    if name == "spin_in_place":
        assert 2 < free[0] < 9 and res[0, 3] == 0  # the long side swings into the block; the origin never moves
    if name == "arcs_not_finite":
        assert free == [0, 0, 0, 0, 4]
    if name.startswith("footprint_"):
        assert free == [0, 0]
    if name == "exact_integer":
        assert free == [0, 2]
    if name == "unreached_and_clamped":
        assert res.tolist() == [[1, 7, 7, ar.UNREACHED], [1, 7, 7, 300]]
    if name == "fuzz_2000":
        assert len(free) == 2000 and min(free) == 0 and max(free) >= 4
    if name == "fuzz_sparse_500":
        assert max(free) == n_steps and min(free) < n_steps


@pytest.mark.parametrize("box", [(-0.5, 0.5, -0.3, 0.3, 0.05), (-0.2, 0.2, -0.1, 0.1, 0.1), (0.0, 1.0, 0.0, 0.0, 0.3), (0.25, 0.25, -1.0, -1.0, 1.0),
                                 (-0.31, 0.77, -0.2, 0.45, 0.07), (0.0, 1.0, 0.0, 1.0, 5.0)])
def test_footprint_box(box):
    got, want = K.footprint_box(*box), ar.footprint_box(*box)
    assert got.dtype == np.float64 and got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    x_min, x_max, y_min, y_max, spacing = box
    nx, ny = math.ceil((x_max - x_min) / spacing) + 1, math.ceil((y_max - y_min) / spacing) + 1
    assert len(got) == nx * ny and got[0].tolist() == [x_min, y_min] and got[-1].tolist() == [x_max, y_max]  # the corners are the box's own
    assert got[nx - 1].tolist() == [x_max, y_min] and got[-nx].tolist() == [x_min, y_max]
    if nx > 1:
        assert (np.diff(got[:nx, 0]) > 0).all() and np.diff(got[:nx, 0]).max() <= spacing * (1 + 1e-12)
    if box == (-0.5, 0.5, -0.3, 0.3, 0.05):
        assert (nx, ny) == (21, 13)
    if box == (0.25, 0.25, -1.0, -1.0, 1.0):
        assert got.tolist() == [[0.25, -1.0]]
    out = np.zeros((nx * ny, 2))
    assert K.footprint_box(*box, out=out) is out and np.array_equal(out, want)


def test_arcs_best():
    U = ar.UNREACHED
    res = np.array([[5, 100, 30, 700], [8, 90, 20, 500], [8, 300, 90, 500], [8, 90, 20, 500], [2, 10, 10, 100], [8, 1, 1, U], [0, 0, 0, 40]], dtype=np.uint32)
    for kw in (dict(), dict(w_cost=1), dict(w_potential=0, w_cost=1), dict(w_potential=0, w_cost=0, w_blocked=1), dict(min_free_steps=3), dict(min_free_steps=0),
               dict(min_free_steps=6, w_blocked=1000), dict(min_free_steps=9), dict(w_potential=0xFFFFFFFF, w_cost=0xFFFFFFFF, w_blocked=0xFFFFFFFF, min_free_steps=0)):
        assert K.arcs_best(res, 8, **kw) == ar.arcs_best(res, 8, **kw), kw
    assert K.arcs_best(res, 8) == 4  # the least potential among those with a free step
    assert K.arcs_best(res, 8, min_free_steps=0) == 6  # the arc that does not move is admissible only then
    assert K.arcs_best(res, 8, min_free_steps=3) == 1  # 1 and 3 tie, and 2 with w_cost = 0: the lowest index
    assert K.arcs_best(res, 8, min_free_steps=3, w_potential=0, w_blocked=1) == 1
    assert K.arcs_best(res, 8, min_free_steps=9) is None  # none admissible
    assert K.arcs_best(res[5:6], 8, min_free_steps=0) is None  # outside the grid, whatever it scores
    big = np.array([[1, 2, 1, 0xFFFFFFFE], [1, 0xFFFFFFFF, 1, 1]], dtype=np.uint32)  # the products need 64 bits: 2^64 - 2^32 - 2 against 2^64 - 2^33 + 1
    assert K.arcs_best(big, 1, w_potential=0xFFFFFFFF, w_cost=0xFFFFFFFE) == 1 == ar.arcs_best(big, 1, w_potential=0xFFFFFFFF, w_cost=0xFFFFFFFE)
    index = C.c_size_t(99)
    assert K.lib().kicp_arcs_best(res.ctypes.data_as(C.POINTER(C.c_uint)), 7, 1, 0, 0, 8, 9, C.byref(index)) == K.KICP_OK and index.value == 7  # *out_index = K


def _code(fn, *a, **kw):
    with pytest.raises(K.KicpError) as e:
        fn(*a, **kw)
    return e.value.code, str(e.value)


def test_argument_and_capacity_errors():
    q, potential, cell, start, arcs, n_steps, footprint, want = ar.pinned_8x6()
    score = lambda **kw: K.score_arcs_from_plan(**{**dict(q=q, potential=potential, cell=cell, origin_x=0.0, origin_y=0.0, start=start, arcs=arcs, n_steps=n_steps,
                                                           footprint=footprint), **kw})
    assert np.array_equal(score(), want)
    for kw in (dict(n_steps=0), dict(n_steps=-1), dict(arcs=np.zeros((0, 4))), dict(footprint=np.zeros((0, 2))), dict(start=(0.75, 0.75, float("nan"), 0.0)),
               dict(start=(float("inf"), 0.75, 1.0, 0.0)), dict(start=(0.75, 0.75, 1.0)), dict(arcs=np.zeros((2, 3))), dict(footprint=np.zeros((3, 3))), dict(cell=0.0),
               dict(cell=float("inf")), dict(cell=-0.5), dict(origin_x=float("nan")), dict(origin_y=float("-inf")), dict(potential=potential[:5]), dict(q=np.zeros((0, 3), np.uint8)),
               dict(out=np.zeros((2, 4), dtype=np.int32)), dict(out=np.zeros((3, 4), dtype=np.uint32)), dict(out=np.zeros((2, 8), dtype=np.uint32)[:, ::2]), dict(out=[0] * 8)):
        assert _code(score, **kw)[0] == K.KICP_ERR_ARG, kw
    for kw, limit in ((dict(n_steps=1025), "1024"), (dict(footprint=np.zeros((4097, 2))), "4096"), (dict(arcs=np.zeros(((1 << 20) + 1, 4))), str(1 << 20))):
        code, msg = _code(score, **kw)
        assert code == K.KICP_ERR_CAPACITY and limit in msg, (kw, msg)
    assert score(n_steps=1024).shape == (2, 4) and score(footprint=np.zeros((4096, 2))).shape == (2, 4)  # the limits themselves are legal
    out = np.zeros((2, 4), dtype=np.uint32)
    assert score(out=out) is out and np.array_equal(out, want)  # written in place

    assert _code(K.arc_steps, [], [], 0.1)[0] == K.KICP_ERR_ARG and _code(K.arc_steps, [1.0], [1.0, 2.0], 0.1)[0] == K.KICP_ERR_ARG
    code, msg = _code(K.arc_steps, np.zeros((1 << 20) + 1), np.zeros((1 << 20) + 1), 0.1)
    assert code == K.KICP_ERR_CAPACITY and str(1 << 20) in msg
    assert _code(K.arc_steps, [1.0], [1.0], 0.1, out=np.zeros((1, 3)))[0] == K.KICP_ERR_ARG
    for box in ((0.5, -0.5, 0.0, 1.0, 0.1), (0.0, 1.0, 1.0, 0.0, 0.1), (0.0, 1.0, 0.0, 1.0, 0.0), (0.0, 1.0, 0.0, 1.0, -0.1), (0.0, float("inf"), 0.0, 1.0, 0.1),
                (float("nan"), 1.0, 0.0, 1.0, 0.1), (0.0, 1.0, 0.0, 1.0, float("nan")), (0.0, 1.0, 0.0, 1.0, float("inf"))):
        assert _code(K.footprint_box, *box)[0] == K.KICP_ERR_ARG, box
    code, msg = _code(K.footprint_box, 0.0, 1.0, 0.0, 1.0, 0.01)  # 101 x 101
    assert code == K.KICP_ERR_CAPACITY and "4096" in msg
    assert _code(K.footprint_box, 0.0, 1.0, 0.0, 1.0, 1e-300)[0] == K.KICP_ERR_CAPACITY
    assert len(K.footprint_box(0.0, 0.63, 0.0, 0.63, 0.01)) == 4096
    assert _code(K.footprint_box, 0.0, 1.0, 0.0, 1.0, 0.5, out=np.zeros((8, 2)))[0] == K.KICP_ERR_ARG
    assert _code(K.arcs_best, np.zeros((0, 4), np.uint32), 8)[0] == K.KICP_ERR_ARG and _code(K.arcs_best, np.zeros((2, 3), np.uint32), 8)[0] == K.KICP_ERR_ARG
    assert _code(K.arcs_best, want, -1)[0] == K.KICP_ERR_ARG and _code(K.arcs_best, want, 4, w_cost=1 << 32)[0] == K.KICP_ERR_ARG
    assert _code(K.plan_q, q, np.zeros(255, np.uint8))[0] == K.KICP_ERR_ARG and _code(K.plan_q, q, pr.IDENTITY, out=np.zeros((6, 8), np.int8))[0] == K.KICP_ERR_ARG

    # the C entries
    lib = K.lib()
    dp, u8, u32 = C.POINTER(C.c_double), C.POINTER(C.c_ubyte), C.POINTER(C.c_uint)
    s, a, f = np.array(start), np.ascontiguousarray(arcs), np.ascontiguousarray(footprint)
    res = np.zeros(8, dtype=np.uint32)
    good = [q.ctypes.data_as(u8), potential.ctypes.data_as(u32), 0.5, 0.0, 0.0, 8, 6, s.ctypes.data_as(dp), a.ctypes.data_as(dp), 2, 4, f.ctypes.data_as(dp), 3, res.ctypes.data_as(u32), 8]
    assert lib.kicp_score_arcs_from_plan(*good) == K.KICP_OK and np.array_equal(res.reshape(2, 4), want)
    for k, v in ((0, None), (1, None), (7, None), (8, None), (11, None), (13, None), (5, 0), (6, 0), (9, 0), (10, 0), (12, 0), (14, 7), (14, 9), (14, 2)):
        bad = list(good)
        bad[k] = v
        assert lib.kicp_score_arcs_from_plan(*bad) == K.KICP_ERR_ARG, k
    for k, v in ((9, (1 << 20) + 1), (10, 1025), (12, 4097)):
        bad = list(good)
        bad[k] = v
        assert lib.kicp_score_arcs_from_plan(*bad) == K.KICP_ERR_CAPACITY, k
    assert lib.kicp_score_arcs_from_plan(*good[:5], 1 << 15, (1 << 13) + 1, *good[7:]) == K.KICP_ERR_CAPACITY
    assert lib.kicp_grid_score_arcs(None, *good[7:]) == K.KICP_ERR_ARG
    v = np.array([1.0, 2.0])
    steps = np.zeros(8)
    assert lib.kicp_arc_steps(v.ctypes.data_as(dp), v.ctypes.data_as(dp), 0.1, 2, steps.ctypes.data_as(dp)) == K.KICP_OK
    for args in ((None, v.ctypes.data_as(dp), 0.1, 2, steps.ctypes.data_as(dp)), (v.ctypes.data_as(dp), None, 0.1, 2, steps.ctypes.data_as(dp)),
                 (v.ctypes.data_as(dp), v.ctypes.data_as(dp), 0.1, 2, None), (v.ctypes.data_as(dp), v.ctypes.data_as(dp), 0.1, 0, steps.ctypes.data_as(dp))):
        assert lib.kicp_arc_steps(*args) == K.KICP_ERR_ARG
    # a buffer that is too small gets the first cap samples and the needed count, as kicp_potential_path does
    xy, n = np.full((20, 2), 77.0), C.c_size_t(99)
    box = (-0.2, 0.2, -0.1, 0.1, 0.1)
    assert lib.kicp_footprint_box(*box, xy.ctypes.data_as(dp), 4, C.byref(n)) == K.KICP_ERR_CAPACITY and n.value == 15
    assert np.array_equal(xy[:4], ar.footprint_box(*box)[:4]) and (xy[4:] == 77.0).all()
    assert lib.kicp_footprint_box(*box, None, 0, C.byref(n)) == K.KICP_ERR_CAPACITY and n.value == 15
    assert lib.kicp_footprint_box(*box, xy.ctypes.data_as(dp), 15, C.byref(n)) == K.KICP_OK and n.value == 15 and (xy[15:] == 77.0).all()
    assert lib.kicp_footprint_box(*box, None, 4, C.byref(n)) == K.KICP_ERR_ARG and lib.kicp_footprint_box(*box, xy.ctypes.data_as(dp), 15, None) == K.KICP_ERR_ARG
    n.value = 5
    assert lib.kicp_footprint_box(0.0, 1.0, 0.0, 1.0, 0.01, xy.ctypes.data_as(dp), 20, C.byref(n)) == K.KICP_ERR_CAPACITY and n.value == 0
    index = C.c_size_t()
    assert lib.kicp_arcs_best(None, 2, 1, 0, 0, 4, 1, C.byref(index)) == K.KICP_ERR_ARG and lib.kicp_arcs_best(res.ctypes.data_as(u32), 2, 1, 0, 0, 4, 1, None) == K.KICP_ERR_ARG
    assert lib.kicp_arcs_best(res.ctypes.data_as(u32), (1 << 20) + 1, 1, 0, 0, 4, 1, C.byref(index)) == K.KICP_ERR_CAPACITY
    w = K.plan_weights()
    assert lib.kicp_plan_q(None, 4, w.ctypes.data_as(u8), res.ctypes.data_as(u8)) == K.KICP_ERR_ARG and lib.kicp_plan_q(q.ctypes.data_as(u8), 4, None, res.ctypes.data_as(u8)) == K.KICP_ERR_ARG
    assert lib.kicp_plan_q(q.ctypes.data_as(u8), 4, w.ctypes.data_as(u8), None) == K.KICP_ERR_ARG and lib.kicp_plan_q(None, 0, w.ctypes.data_as(u8), None) == K.KICP_OK


def _build(tmp_path, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", include, "-I",
                           os.path.join(ROOT, "kinematic_icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "arcs_host_test.cpp"), "-o", exe] + extra)
    return exe


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_arcs_host_stand_alone(tmp_path, reference, flags):
    """arcs_host:: in a program of its own (tests/cpp/arcs_host_test.cpp), as a subprocess; the sanitizers run on this host program
    only.  The box's buffer holds exactly its samples - or four, to see a short buffer handled"""
    exe = _build(tmp_path, "arcs_host_test", flags)
    boxes = [(-0.5, 0.5, -0.3, 0.3, 0.05), (-0.2, 0.2, -0.1, 0.1, 0.1), (0.25, 0.25, -1.0, -1.0, 1.0)]
    ranks = [(1, 0, 0, 1), (1, 2, 300, 0), (0, 1, 0, 3)]
    rng = np.random.Generator(np.random.PCG64(3))
    runs = 0
    for k, (name, case) in enumerate(sorted(CASES.items())):
        q, goals, max_potential, cell, ox, oy, start, arcs, n_steps, footprint = case
        pot, want = reference[name]
        H, W = q.shape
        box, rank = boxes[k % len(boxes)], ranks[k % len(ranks)]
        box_want = ar.footprint_box(*box)
        cap = 4 if k % 4 == 3 else len(box_want)
        v, omega = rng.uniform(-2.0, 2.0, len(arcs)), rng.uniform(-3.0, 3.0, len(arcs))
        omega[0] = 1e-10
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            np.array([W, H, cell, ox, oy, len(arcs), n_steps, len(footprint), 0.1] + list(box) + [cap] + list(rank), dtype=np.float64).tofile(f)
            np.array(start, dtype=np.float64).tofile(f), np.ascontiguousarray(arcs, dtype=np.float64).tofile(f), np.ascontiguousarray(footprint, dtype=np.float64).tofile(f)
            v.tofile(f), omega.tofile(f), np.ascontiguousarray(q).tofile(f), np.ascontiguousarray(pot).tofile(f)
        out = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert out.returncode == 0, (name, (out.stdout + out.stderr)[-2000:])
        raw = open(dst, "rb").read()
        n = len(arcs)
        assert np.array_equal(np.frombuffer(raw[:16 * n], dtype=np.uint32).reshape(n, 4), want), name
        assert np.array_equal(np.frombuffer(raw[16 * n:48 * n], dtype=np.uint64), ar.arc_steps(v, omega, 0.1).view(np.uint64).reshape(-1)), name
        assert np.frombuffer(raw[48 * n:48 * n + 8], dtype=np.uint64)[0] == len(box_want)
        stored = min(cap, len(box_want))
        assert np.array_equal(np.frombuffer(raw[48 * n + 8:48 * n + 8 + 16 * stored], dtype=np.float64).reshape(stored, 2), box_want[:stored])
        best = ar.arcs_best(want, n_steps, *rank)
        assert len(raw) == 48 * n + 16 + 16 * stored and np.frombuffer(raw[-8:], dtype=np.uint64)[0] == (n if best is None else best), name
        runs += 1
    assert runs >= 20
