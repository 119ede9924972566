"""Scoring a tree of arc segments without a GPU: the pure-host entries (K.score_arc_tree_from_plan, K.arc_tree_nodes, K.arc_tree_best)
against the restatement of include/kicp.h's text in Python floats (tests/arc_tree_ref.py, which rolls every node from the start on its
own) - np.array_equal, no tolerance - a pinned 8 x 6 case with its rows written out, a tree of depth 1 against K.score_arcs_from_plan,
the limits and the argument errors, and the shared header (kicp_arc_tree_host.hpp: the very arithmetic the kernel calls) in a
stand-alone program, built plainly and under ASan + UBSan, on the same cases."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
import arcs_ref as ar
import arc_tree_ref as tr
import potential_ref as pr

CASES = tr.small_cases()


@pytest.fixture(scope="module")
def reference():
    """name -> (potential, rows by the restatement, the nodes' classes) - computed once"""
    out = {}
    for name, case in CASES.items():
        q, goals, max_potential = case[:3]
        pot = K.potential_from_costmap(q, pr.IDENTITY, goals, max_potential)
        out[name] = (pot,) + tr.score_tree(q, pot, *case[3:], return_classes=True)
    return out


def test_pinned_8x6_tree():
    q, potential, cell, start, _, _, footprint, _ = ar.pinned_8x6()
    branch, steps, primitives, want = tr.pinned_8x6_tree()
    assert want.tolist() == [[1, 10, 10, 102], [1, 10, 10, 102], [2, 60, 50, 103], [3, 70, 30, 203], [3, 40, 20, 302], [3, 50, 20, 201]]
    assert np.array_equal(tr.score_tree(q, potential, cell, 0.0, 0.0, start, branch, steps, primitives, footprint), want)
    got = K.score_arc_tree_from_plan(q, potential, cell, 0.0, 0.0, start, branch, steps, primitives, footprint)
    assert got.dtype == np.uint32 and got.shape == (6, 4) and np.array_equal(got, want)
    assert K.arc_tree_nodes(branch, steps) == (6, 4, 3, (0, 2))
    assert K.arc_tree_best(want, branch, steps) == (0, (0, 0))  # the least potential: straight on, and it stops short of the wall
    assert K.arc_tree_best(want, branch, steps, min_free_steps=3) == (3, (1, 1))  # among the three that took every step
    assert K.arc_tree_best(want, branch, steps, w_potential=0, w_cost=1) == (2, (1, 0))
    out = np.zeros((6, 4), dtype=np.uint32)
    assert K.score_arc_tree_from_plan(q, potential, cell, 0.0, 0.0, start, branch, steps, primitives, footprint, out=out) is out and np.array_equal(out, want)


@pytest.mark.parametrize("name", sorted(CASES))
def test_score_arc_tree_from_plan(name, reference):
    q, goals, max_potential, cell, ox, oy, start, branch, steps, primitives, footprint = CASES[name]
    pot, want, classes = reference[name]
    got = K.score_arc_tree_from_plan(q, pot, cell, ox, oy, start, branch, steps, primitives, footprint)
    assert got.dtype == np.uint32 and got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:5]
    tr.check_case(name, want, classes, branch, steps, pot)
    free, total, largest = want[:, 0].astype(int), want[:, 1].astype(int), want[:, 2].astype(int)
    assert (largest * free >= total).all() and (total >= largest).all() and ((free == 0) == (largest == 0)).all()
    n_nodes, n_leaves, total_steps, offsets = K.arc_tree_nodes(branch, steps)
    assert (n_nodes, n_leaves, total_steps, offsets) == tr.nodes(branch, steps)
    # a node under one that ended early repeats its words; an alive node took every step of its path
    ends = offsets[1:] + (n_nodes,)
    for level in range(1, len(branch)):
        parents, children = want[offsets[level - 1]:ends[level - 1]], want[offsets[level]:ends[level]]
        inherited = classes[offsets[level]:ends[level]] == tr.INHERITED
        assert np.array_equal(children[inherited], np.repeat(parents, branch[level], axis=0)[inherited])
    path_steps = np.repeat(np.cumsum(steps), np.subtract(ends, offsets))
    assert (free[classes == tr.ALIVE] == path_steps[classes == tr.ALIVE]).all() and (free[classes != tr.ALIVE] < path_steps[classes != tr.ALIVE]).all()


@pytest.mark.parametrize("name", ["depth_1_of_%d" % n for n in (1, 3, 4, 5, 257)])
def test_depth_1_equals_score_arcs_from_plan(name, reference):
    q, goals, max_potential, cell, ox, oy, start, branch, steps, primitives, footprint = CASES[name]
    pot, want, _ = reference[name]
    arcs = K.score_arcs_from_plan(q, pot, cell, ox, oy, start, primitives, steps[0], footprint)
    assert np.array_equal(arcs, want) and np.array_equal(arcs, ar.score_arcs(q, pot, cell, ox, oy, start, primitives, steps[0], footprint))
    best = K.arc_tree_best(want, branch, steps)
    index = K.arcs_best(want, steps[0])
    assert best == (None if index is None else (index, (index,)))


def test_arc_tree_best():
    U = ar.UNREACHED
    branch, steps = (2, 3), (3, 5)  # 2 + 6 rows, T = 8; level 1's rows would win every ranking and must not be looked at
    res = np.array([[8, 0, 0, 1], [8, 0, 0, 1],
                    [5, 100, 30, 700], [8, 90, 20, 500], [8, 300, 90, 500], [8, 90, 20, 500], [2, 10, 10, 100], [8, 1, 1, U]], dtype=np.uint32)
    for kw in (dict(), dict(w_cost=1), dict(w_potential=0, w_cost=1), dict(w_potential=0, w_cost=0, w_blocked=1), dict(min_free_steps=3), dict(min_free_steps=0),
               dict(min_free_steps=6, w_blocked=1000), dict(min_free_steps=9), dict(w_potential=0xFFFFFFFF, w_cost=0xFFFFFFFF, w_blocked=0xFFFFFFFF, min_free_steps=0)):
        assert K.arc_tree_best(res, branch, steps, **kw) == tr.best(res, branch, steps, **kw), kw
    assert K.arc_tree_best(res, branch, steps) == (4, (1, 1))  # the least potential among the leaves with a free step
    assert K.arc_tree_best(res, branch, steps, min_free_steps=3) == (1, (0, 1))  # leaves 1 and 3 tie, and 2 with w_cost = 0: the lowest index
    assert K.arc_tree_best(res, branch, steps, min_free_steps=3, w_potential=0, w_blocked=1) == (1, (0, 1))  # blocked counts against T = 8
    assert K.arc_tree_best(res, branch, steps, w_potential=0, w_blocked=1) == (1, (0, 1)) and K.arc_tree_best(res, branch, steps, w_potential=0, w_cost=1, w_blocked=20) == (1, (0, 1))
    assert K.arc_tree_best(res, branch, steps, min_free_steps=9) is None  # none admissible
    deep = (2, 1, 3, 2)  # 2 + 2 + 6 + 12 rows: the path of leaf 7 is (1, 0, 0, 1) - 7 = ((1 * 1 + 0) * 3 + 0) * 2 + 1
    rows = np.zeros((22, 4), dtype=np.uint32)
    rows[:, 3] = 50
    rows[:, 0] = 4
    rows[10 + 7, 3] = 9
    assert K.arc_tree_best(rows, deep, (1, 1, 1, 1)) == (7, (1, 0, 0, 1)) == tr.best(rows, deep, (1, 1, 1, 1))
    leaf, path = C.c_size_t(99), np.full(2, 77, dtype=np.uint32)
    b, s = np.array(branch, dtype=np.uint32), np.array(steps, dtype=np.uint32)
    u32 = C.POINTER(C.c_uint)
    assert K.lib().kicp_arc_tree_best(res.ctypes.data_as(u32), 2, b.ctypes.data_as(u32), s.ctypes.data_as(u32), 1, 0, 0, 9, C.byref(leaf), path.ctypes.data_as(u32)) == K.KICP_OK
    assert leaf.value == 6 and path.tolist() == [77, 77]  # *out_leaf = n_D, and no path is written


def _code(fn, *a, **kw):
    with pytest.raises(K.KicpError) as e:
        fn(*a, **kw)
    return e.value.code, str(e.value)


def test_arc_tree_nodes_at_the_limits():
    assert K.arc_tree_nodes((1024, 1023), (1, 1)) == (1 << 20, 1024 * 1023, 2, (0, 1024)) == tr.nodes((1024, 1023), (1, 1))  # exactly 2^20 nodes
    assert K.arc_tree_nodes((1 << 20,), (1024,)) == (1 << 20, 1 << 20, 1024, (0,))
    assert K.arc_tree_nodes((2,) * 8, (128,) * 8) == (510, 256, 1024, (0, 2, 6, 14, 30, 62, 126, 254))  # steps summing to 1 024
    assert K.arc_tree_nodes((8, 8, 8, 8), (8,) * 4)[:3] == (4680, 4096, 32)
    for branch, steps, limit in (((1024, 1024), (1, 1), str(1 << 20)), (((1 << 20) + 1,), (1,), str(1 << 20)), ((0xFFFFFFFF,) * 8, (1,) * 8, str(1 << 20)),
                                 ((1, 1), (1000, 25), "1024"), ((2,) * 8, (128,) * 7 + (129,), "1024"), ((1,), (0xFFFFFFFF,), "1024"), ((1,) * 8, (0xFFFFFFFF,) * 8, "1024"),
                                 ((1,) * 9, (1,) * 9, "8")):
        code, msg = _code(K.arc_tree_nodes, branch, steps)
        assert code == K.KICP_ERR_CAPACITY and limit in msg and tr.nodes(branch, steps) == "capacity", (branch, steps, msg)
    for branch, steps in (((), ()), ((2, 0), (1, 1)), ((2, 2), (1, 0)), ((0,), (1,)), ((2, 2), (1,)), ((-1,), (1,)), ((2,), (1 << 32,)), ((1.5,), (1,))):
        assert _code(K.arc_tree_nodes, branch, steps)[0] == K.KICP_ERR_ARG, (branch, steps)
    lib = K.lib()
    u32, sz = C.POINTER(C.c_uint), C.POINTER(C.c_size_t)
    b, s = np.array([3, 4], dtype=np.uint32), np.array([5, 6], dtype=np.uint32)
    n, leaves, total, offsets = C.c_size_t(9), C.c_size_t(9), C.c_uint(9), (C.c_size_t * 2)(9, 9)
    good = [2, b.ctypes.data_as(u32), s.ctypes.data_as(u32), C.byref(n), C.byref(leaves), C.byref(total), offsets]
    assert lib.kicp_arc_tree_nodes(*good) == K.KICP_OK and (n.value, leaves.value, total.value, list(offsets)) == (15, 12, 11, [0, 3])
    assert lib.kicp_arc_tree_nodes(*good[:6], None) == K.KICP_OK  # the offsets may be left out
    for k in (1, 2, 3, 4, 5):
        bad = list(good)
        bad[k] = None
        assert lib.kicp_arc_tree_nodes(*bad) == K.KICP_ERR_ARG, k
    assert lib.kicp_arc_tree_nodes(0, *good[1:]) == K.KICP_ERR_ARG and (n.value, leaves.value, total.value) == (0, 0, 0)
    assert lib.kicp_arc_tree_nodes(9, *good[1:]) == K.KICP_ERR_CAPACITY


def test_argument_and_capacity_errors():
    q, potential, cell, start, _, _, footprint, _ = ar.pinned_8x6()
    branch, steps, primitives, want = tr.pinned_8x6_tree()
    score = lambda **kw: K.score_arc_tree_from_plan(**{**dict(q=q, potential=potential, cell=cell, origin_x=0.0, origin_y=0.0, start=start, branch=branch, steps=steps,
                                                               primitives=primitives, footprint=footprint), **kw})
    assert np.array_equal(score(), want)
    for kw in (dict(branch=(), steps=()), dict(branch=(2, 0)), dict(steps=(1, 0)), dict(steps=(1,)), dict(branch=(2, -2)), dict(primitives=primitives[:3]),
               dict(primitives=np.zeros((5, 4))), dict(primitives=np.zeros((4, 3))), dict(primitives=np.zeros(16)), dict(footprint=np.zeros((0, 2))),
               dict(footprint=np.zeros((3, 3))), dict(start=(0.75, 0.75, float("nan"), 0.0)), dict(start=(float("inf"), 0.75, 1.0, 0.0)), dict(start=(0.75, 0.75, 1.0)),
               dict(cell=0.0), dict(cell=float("inf")), dict(origin_x=float("nan")), dict(potential=potential[:5]), dict(q=np.zeros((0, 3), np.uint8)),
               dict(out=np.zeros((6, 4), dtype=np.int32)), dict(out=np.zeros((4, 4), dtype=np.uint32)), dict(out=np.zeros((6, 8), dtype=np.uint32)[:, ::2]), dict(out=[0] * 24)):
        assert _code(score, **kw)[0] == K.KICP_ERR_ARG, kw
    for kw, limit in ((dict(steps=(1000, 25)), "1024"), (dict(footprint=np.zeros((4097, 2))), "4096"), (dict(branch=(1024, 1024), primitives=np.zeros((2048, 4))), str(1 << 20)),
                      (dict(branch=(1,) * 9, steps=(1,) * 9, primitives=np.zeros((9, 4))), "8")):
        code, msg = _code(score, **kw)
        assert code == K.KICP_ERR_CAPACITY and limit in msg, (kw, msg)
    assert score(steps=(1000, 24)).shape == (6, 4) and score(footprint=np.zeros((4096, 2))).shape == (6, 4)  # the limits themselves are legal
    assert _code(K.arc_tree_best, want[:5], branch, steps)[0] == K.KICP_ERR_ARG and _code(K.arc_tree_best, want, branch, (1, 0))[0] == K.KICP_ERR_ARG
    assert _code(K.arc_tree_best, want, branch, steps, w_cost=1 << 32)[0] == K.KICP_ERR_ARG and _code(K.arc_tree_best, want, branch, steps, min_free_steps=-1)[0] == K.KICP_ERR_ARG

    # the C entries
    lib = K.lib()
    dp, u8, u32 = C.POINTER(C.c_double), C.POINTER(C.c_ubyte), C.POINTER(C.c_uint)
    s, p, f = np.array(start), np.ascontiguousarray(primitives), np.ascontiguousarray(footprint)
    b, st = np.array(branch, dtype=np.uint32), np.array(steps, dtype=np.uint32)
    res = np.zeros(24, dtype=np.uint32)
    good = [q.ctypes.data_as(u8), potential.ctypes.data_as(u32), 0.5, 0.0, 0.0, 8, 6, s.ctypes.data_as(dp), 2, b.ctypes.data_as(u32), st.ctypes.data_as(u32), p.ctypes.data_as(dp),
            f.ctypes.data_as(dp), 3, res.ctypes.data_as(u32), 24]
    assert lib.kicp_score_arc_tree_from_plan(*good) == K.KICP_OK and np.array_equal(res.reshape(6, 4), want)
    for k, v in ((0, None), (1, None), (7, None), (9, None), (10, None), (11, None), (12, None), (14, None), (5, 0), (6, 0), (8, 0), (13, 0), (15, 23), (15, 25), (15, 16), (15, 6)):
        bad = list(good)
        bad[k] = v
        assert lib.kicp_score_arc_tree_from_plan(*bad) == K.KICP_ERR_ARG, k
    for k, v in ((8, 9), (13, 4097)):
        bad = list(good)
        bad[k] = v
        assert lib.kicp_score_arc_tree_from_plan(*bad) == K.KICP_ERR_CAPACITY, k
    assert lib.kicp_grid_score_arc_tree(None, *good[7:]) == K.KICP_ERR_ARG
    leaf, path = C.c_size_t(), np.zeros(2, dtype=np.uint32)
    best = [res.ctypes.data_as(u32), 2, b.ctypes.data_as(u32), st.ctypes.data_as(u32), 1, 0, 0, 1, C.byref(leaf), path.ctypes.data_as(u32)]
    assert lib.kicp_arc_tree_best(*best) == K.KICP_OK and (leaf.value, path.tolist()) == (0, [0, 0])
    for k in (0, 2, 3, 8, 9):
        bad = list(best)
        bad[k] = None
        assert lib.kicp_arc_tree_best(*bad) == K.KICP_ERR_ARG, k
    assert lib.kicp_arc_tree_best(best[0], 0, *best[2:]) == K.KICP_ERR_ARG and lib.kicp_arc_tree_best(best[0], 9, *best[2:]) == K.KICP_ERR_CAPACITY


def _build(tmp_path, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", include, "-I",
                           os.path.join(ROOT, "kinematic_icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "arc_tree_host_test.cpp"), "-o", exe] + extra)
    return exe


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_arc_tree_host_stand_alone(tmp_path, reference, flags):
    """arc_tree_host:: in a program of its own (tests/cpp/arc_tree_host_test.cpp), as a subprocess; the sanitizers run on this host
    program only.  Its buffers hold exactly the rows and exactly the records of the widest level above the leaves"""
    exe = _build(tmp_path, "arc_tree_host_test", flags)
    ranks = [(1, 0, 0, 1), (1, 2, 300, 0), (0, 1, 0, 3), (1, 0, 0, 1025)]
    runs = 0
    for k, (name, case) in enumerate(sorted(CASES.items())):
        q, goals, max_potential, cell, ox, oy, start, branch, steps, primitives, footprint = case
        pot, want, _ = reference[name]
        H, W = q.shape
        D, rank = len(branch), ranks[k % len(ranks)]
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            np.array([W, H, cell, ox, oy, D, len(footprint)] + list(rank) + list(branch) + list(steps), dtype=np.float64).tofile(f)
            np.array(start, dtype=np.float64).tofile(f), np.ascontiguousarray(primitives, dtype=np.float64).tofile(f), np.ascontiguousarray(footprint, dtype=np.float64).tofile(f)
            np.ascontiguousarray(q).tofile(f), np.ascontiguousarray(pot).tofile(f)
        out = subprocess.run([exe, src, dst], capture_output=True, text=True)
        assert out.returncode == 0, (name, (out.stdout + out.stderr)[-2000:])
        raw = open(dst, "rb").read()
        n_nodes, n_leaves, total, offsets = tr.nodes(branch, steps)
        head = 8 * (3 + D)
        assert np.frombuffer(raw[:head], dtype=np.uint64).tolist() == [n_nodes, n_leaves, total] + list(offsets), name
        assert np.array_equal(np.frombuffer(raw[head:head + 16 * n_nodes], dtype=np.uint32).reshape(n_nodes, 4), want), name
        best = tr.best(want, branch, steps, *rank)
        tail = raw[head + 16 * n_nodes:]
        assert len(tail) == 8 + 4 * D and np.frombuffer(tail[:8], dtype=np.uint64)[0] == (n_leaves if best is None else best[0]), name
        assert np.frombuffer(tail[8:], dtype=np.uint32).tolist() == ([0xFFFFFFFF] * D if best is None else list(best[1])), name
        runs += 1
    assert runs >= 20
