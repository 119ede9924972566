"""The cost-to-go field and its path without a GPU: the pure-host entries (K.plan_weights, K.potential_from_costmap, K.potential_path)
against the restatement of include/kicp.h's text (tests/potential_ref.py: a heap Dijkstra and numpy min-plus sweeps, which must agree) -
np.array_equal, no tolerance - a pinned 8 x 6 case with its numbers written out, the path rule, the argument errors, and the shared
header (kicp_nav_host.hpp: the very arithmetic the kernels call) in a stand-alone program, built plainly and under ASan + UBSan, on
the same cases."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import kinematic_icp_amd as K
from conftest import ROOT
import potential_ref as pr

CASES = pr.small_cases()


@pytest.fixture(scope="module")
def reference():
    """name -> (potential, stats) by the restatement's Dijkstra - computed once"""
    return {name: pr.potential_dijkstra(*case) for name, case in CASES.items()}


def test_pinned_8x6_case():
    costmap, weight, goals, want = pr.pinned_8x6()
    for got, stats in (pr.potential_dijkstra(costmap, weight, goals), pr.potential_sweeps(costmap, weight, goals)[:2],
                       K.potential_from_costmap(costmap, weight, goals, return_stats=True)):
        assert np.array_equal(got, want) and tuple(stats[:3]) == (1, 42, 0)
    assert pr.edge(1, 1, False) == 2 and pr.edge(1, 1, True) == 3 and pr.edge(1, 5, False) == 6 and pr.edge(5, 1, True) == 8 and pr.edge(255, 255, True) == 721
    clamped = np.where(want == pr.UNREACHED, want, np.minimum(want, 17))
    got, stats = K.potential_from_costmap(costmap, weight, goals, 17, return_stats=True)
    assert np.array_equal(got, clamped) and stats == (1, 34, 8, 0)
    assert np.array_equal(pr.potential_sweeps(costmap, weight, goals, 17)[0], clamped)
    # the path from the far corner: -x comes first along the top row, then the diagonals round the wall's left end, then -y
    cells = K.potential_path(want, costmap, weight, (7, 5))
    assert cells.dtype == np.uint32 and cells.tolist() == [[7, 5], [6, 5], [5, 5], [4, 5], [3, 5], [2, 4], [1, 3], [0, 2], [0, 1], [0, 0]]
    assert K.potential_path(want, costmap, weight, (0, 0)).tolist() == [[0, 0]]


@pytest.mark.parametrize("name", sorted(CASES))
def test_potential_from_costmap(name, reference):
    costmap, weight, goals, max_potential = CASES[name]
    want, want_stats = reference[name]
    swept, swept_stats, _ = pr.potential_sweeps(costmap, weight, goals, max_potential)
    assert np.array_equal(swept, want) and swept_stats == want_stats  # the restatement's two ways agree
    got, stats = K.potential_from_costmap(costmap, weight, goals, max_potential, return_stats=True)
    assert got.dtype == np.uint32 and got.shape == costmap.shape and np.array_equal(got, want)
    assert stats == want_stats + (0,)
    q = np.asarray(weight)[costmap]
    assert (got[q == 0] == pr.UNREACHED).all() and (got[got != pr.UNREACHED] <= max_potential).all()
    assert all(got[y, x] == 0 for x, y in goals if q[y, x] > 0) and (got == 0).sum() == len({g for g in goals if q[g[1], g[0]] > 0})
    if name == "goal_impassable_alone":
        assert (got == pr.UNREACHED).all() and stats[0] == 0
    if name == "enclosed":
        assert (got[11:22, 13:24] == pr.UNREACHED).all()
    if name == "nav2_weights":
        assert (got[costmap >= 253] == pr.UNREACHED).all() and stats[1] > 1000
    if name == "nav2_weights_through_unknown":
        assert (got[costmap == 255] != pr.UNREACHED).any() and stats[0] == 2  # a cell listed twice counts twice
    if name == "random_96x70_clamp_1":
        assert stats[1] == 1 and stats[2] > 4000


@pytest.mark.parametrize("args", [(), (50, 4, 5, 253, 0), (1, 0, 1, 255, 255), (255, 1, 1, 254, 7), (10, 3, 2, 0, 9), (20, 0xFFFFFFFF, 1, 100, 0), (7, 10, 0xFFFFFFFF, 200, 1)])
def test_plan_weights(args):
    got = K.plan_weights(*args)
    assert got.dtype == np.uint8 and got.shape == (256,) and np.array_equal(got, pr.weights(*args))
    neutral, _, _, lethal_from, unknown = args or (50, 4, 5, 253, 0)
    assert got[255] == unknown and (got[lethal_from:255] == 0).all() and (got[:lethal_from] >= neutral).all() and (np.diff(got[:lethal_from].astype(int)) >= 0).all()
    if not args:
        assert got[0] == 50 and got[1] == 50 and got[2] == 51 and got[252] == 251 and got[253] == 0 and got[254] == 0


def _path_checks(pot, costmap, weight, goals, start):
    cells = [tuple(int(v) for v in c) for c in K.potential_path(pot, costmap, weight, start)]
    assert cells == pr.path(pot, costmap, weight, start) and cells[0] == tuple(start) and cells[-1] in goals and pot[cells[-1][1], cells[-1][0]] == 0
    q = np.asarray(weight)[costmap].astype(int)
    for (ax, ay), (bx, by) in zip(cells, cells[1:]):
        assert max(abs(ax - bx), abs(ay - by)) == 1
        assert int(pot[ay, ax]) == int(pot[by, bx]) + pr.edge(q[ay, ax], q[by, bx], ax != bx and ay != by)  # every step satisfies the equality
    return cells


def test_paths(reference):
    for name in ("random_96x70", "nav2_weights", "corners_65x63", "diagonal_across_four_tiles", "enclosed"):
        costmap, weight, goals, _ = CASES[name]
        pot = reference[name][0]
        ys, xs = np.nonzero(pot != pr.UNREACHED)
        for k in range(0, len(xs), max(len(xs) // 25, 1)):
            _path_checks(pot, costmap, weight, goals, (int(xs[k]), int(ys[k])))
    assert _path_checks(reference["diagonal_across_four_tiles"][0], *CASES["diagonal_across_four_tiles"][:3], (31, 31)) == [(31, 31), (32, 32)]
    costmap = pr.serpentine()
    pot = K.potential_from_costmap(costmap, pr.IDENTITY, [(0, 0)])
    assert len(_path_checks(pot, costmap, pr.IDENTITY, [(0, 0)], (129, 99))) > 25 * 125


def test_tie_break_order_on_an_open_field():
    """every cell weighs 1: many shortest paths, and the rule's order - +x, -x, +y, -y, then the diagonals - picks one"""
    costmap = np.ones((9, 12), dtype=np.uint8)
    pot = K.potential_from_costmap(costmap, pr.IDENTITY, [(5, 2)])
    assert pot[0, 0] == 3 * 2 + 2 * 3
    assert K.potential_path(pot, costmap, pr.IDENTITY, (0, 0)).tolist() == [[0, 0], [1, 0], [2, 0], [3, 0], [4, 1], [5, 2]]  # +x while it descends
    assert K.potential_path(pot, costmap, pr.IDENTITY, (11, 8)).tolist() == [list(c) for c in pr.path(pot, costmap, pr.IDENTITY, (11, 8))]
    assert K.potential_path(pot, costmap, pr.IDENTITY, (8, 0)).tolist() == [[8, 0], [7, 0], [6, 1], [5, 2]]  # -x before +y and before the diagonals
    assert K.potential_path(pot, costmap, pr.IDENTITY, (3, 7)).tolist() == [[3, 7], [3, 6], [3, 5], [3, 4], [4, 3], [5, 2]]  # -y (the fourth) before (+x, -y)
    assert K.potential_path(pot, costmap, pr.IDENTITY, (5, 0)).tolist() == [[5, 0], [5, 1], [5, 2]]


def _code(fn, *a, **kw):
    with pytest.raises(K.KicpError) as e:
        fn(*a, **kw)
    return e.value.code, str(e.value)


def test_path_errors(reference):
    costmap, weight, goals, _ = CASES["enclosed"]
    pot = reference["enclosed"][0]
    code, msg = _code(K.potential_path, pot, costmap, weight, (18, 16))  # inside the ring
    assert code == K.KICP_ERR_ARG and "unreachable" in msg
    assert _code(K.potential_path, pot, costmap, weight, (12, 15))[0] == K.KICP_ERR_ARG  # on the ring: impassable
    costmap, weight, goals, max_potential = CASES["random_96x70_clamped"]
    pot = reference["random_96x70_clamped"][0]
    ys, xs = np.nonzero(pot == max_potential)
    inside = [(int(x), int(y)) for x, y in zip(xs, ys) if pr.path(pot, costmap, weight, (int(x), int(y))) == "clamped"]
    assert len(inside) > 1000
    for start in inside[::200]:
        code, msg = _code(K.potential_path, pot, costmap, weight, start)
        assert code == K.KICP_ERR_CAPACITY and "max_potential" in msg
    ys, xs = np.nonzero(pot < max_potential)
    _path_checks(pot, costmap, weight, goals, (int(xs[-1]), int(ys[-1])))  # below the clamp the path is there
    for start in ((96, 0), (0, 70), (-1, 0)):
        assert _code(K.potential_path, pot, costmap, weight, start)[0] == K.KICP_ERR_ARG
    assert _code(K.potential_path, pot[:5], costmap, weight, (0, 0))[0] == K.KICP_ERR_ARG

    # the C entry: a buffer that is too small gets the first cap_cells cells and the needed length
    lib = K.lib()
    costmap, weight, goals, want = pr.pinned_8x6()
    u8, u32 = C.POINTER(C.c_ubyte), C.POINTER(C.c_uint)
    out, n = np.full((12, 2), 77, dtype=np.uint32), C.c_size_t(99)
    args = (want.ctypes.data_as(u32), costmap.ctypes.data_as(u8), 8, 6, weight.ctypes.data_as(u8), 7, 5)
    assert lib.kicp_potential_path(*args, out.ctypes.data_as(u32), 3, C.byref(n)) == K.KICP_ERR_CAPACITY
    assert n.value == 10 and out[:3].tolist() == [[7, 5], [6, 5], [5, 5]] and (out[3:] == 77).all()
    assert lib.kicp_potential_path(*args, None, 0, C.byref(n)) == K.KICP_ERR_CAPACITY and n.value == 10
    assert lib.kicp_potential_path(*args, out.ctypes.data_as(u32), 10, C.byref(n)) == K.KICP_OK and n.value == 10 and (out[10:] == 77).all()
    assert lib.kicp_potential_path(*args, None, 3, C.byref(n)) == K.KICP_ERR_ARG
    assert lib.kicp_potential_path(*args, out.ctypes.data_as(u32), 11, None) == K.KICP_ERR_ARG
    for k in (0, 1, 4):
        bad = list(args)
        bad[k] = None
        assert lib.kicp_potential_path(*bad, out.ctypes.data_as(u32), 11, C.byref(n)) == K.KICP_ERR_ARG
    assert lib.kicp_potential_path(*args[:2], 0, 6, *args[4:], out.ctypes.data_as(u32), 11, C.byref(n)) == K.KICP_ERR_ARG
    n.value = 5
    assert lib.kicp_potential_path(*args[:5], 1, 2, out.ctypes.data_as(u32), 11, C.byref(n)) == K.KICP_ERR_ARG and n.value == 0  # on the wall


def test_argument_errors():
    costmap = np.zeros((4, 6), dtype=np.uint8)
    weight = K.plan_weights()
    for goals in ([(6, 0)], [(0, 4)], [(0, 0), (7, 7)], [], [(-1, 0)]):
        assert _code(K.potential_from_costmap, costmap, weight, goals)[0] == K.KICP_ERR_ARG, goals
    for max_potential in (0, 0xFFFFFFFF, -1, 1 << 32):
        assert _code(K.potential_from_costmap, costmap, weight, [(0, 0)], max_potential)[0] == K.KICP_ERR_ARG
    assert K.potential_from_costmap(costmap, weight, [(0, 0)], 1).max() == 1 and K.potential_from_costmap(costmap, weight, [(0, 0)], 0xFFFFFFFE)[3, 5] == 3 * 141 + 2 * 100
    for bad in (np.zeros((0, 4), np.uint8), np.zeros(4, np.uint8), np.zeros((2, 2, 2), np.uint8)):
        assert _code(K.potential_from_costmap, bad, weight, [(0, 0)])[0] == K.KICP_ERR_ARG
    assert _code(K.potential_from_costmap, costmap, weight[:255], [(0, 0)])[0] == K.KICP_ERR_ARG
    out = np.zeros((4, 6), dtype=np.uint32)
    assert K.potential_from_costmap(costmap, weight, [(0, 0)], out=out) is out and out[3, 5] == 3 * 141 + 2 * 100  # written in place
    for bad in (np.zeros((4, 6), dtype=np.int32), np.zeros((6, 4), dtype=np.uint32), np.zeros((4, 12), dtype=np.uint32)[:, ::2], [0] * 24):
        assert _code(K.potential_from_costmap, costmap, weight, [(0, 0)], out=bad)[0] == K.KICP_ERR_ARG
    for kw in (dict(neutral=0), dict(neutral=256), dict(factor_den=0), dict(lethal_from=256), dict(unknown_weight=256), dict(factor_num=-1), dict(neutral=1 << 32)):
        assert _code(K.plan_weights, **kw)[0] == K.KICP_ERR_ARG, kw

    lib = K.lib()
    u8, u32, u64 = C.POINTER(C.c_ubyte), C.POINTER(C.c_uint), C.POINTER(C.c_ulonglong)
    plan = K.PlanConfig(1000)
    goals, out, stats = np.array([[1, 1]], dtype=np.uint32), np.zeros(24, dtype=np.uint32), np.zeros(4, dtype=np.uint64)
    pc, pw, pg, po, ps = costmap.ctypes.data_as(u8), weight.ctypes.data_as(u8), goals.ctypes.data_as(u32), out.ctypes.data_as(u32), stats.ctypes.data_as(u64)
    assert lib.kicp_potential_from_costmap(pc, 6, 4, pw, C.byref(plan), pg, 1, po, 24, ps) == K.KICP_OK and stats.tolist() == [1, 24, 0, 0]
    assert lib.kicp_potential_from_costmap(pc, 6, 4, pw, C.byref(plan), pg, 1, po, 24, None) == K.KICP_OK  # the statistics are optional
    for args in ((None, 6, 4, pw, C.byref(plan), pg, 1, po, 24, ps), (pc, 6, 4, None, C.byref(plan), pg, 1, po, 24, ps), (pc, 6, 4, pw, None, pg, 1, po, 24, ps),
                 (pc, 6, 4, pw, C.byref(plan), None, 1, po, 24, ps), (pc, 6, 4, pw, C.byref(plan), pg, 1, None, 24, ps), (pc, 6, 4, pw, C.byref(plan), pg, 1, po, 23, ps),
                 (pc, 6, 4, pw, C.byref(plan), pg, 1, po, 25, ps), (pc, 6, 4, pw, C.byref(plan), pg, 0, po, 24, ps), (pc, 0, 4, pw, C.byref(plan), pg, 1, po, 0, ps),
                 (pc, 6, 0, pw, C.byref(plan), pg, 1, po, 0, ps), (pc, 1, 1, pw, C.byref(plan), pg, 1, po, 1, ps)):
        assert lib.kicp_potential_from_costmap(*args) == K.KICP_ERR_ARG
    assert lib.kicp_potential_from_costmap(pc, 1 << 15, (1 << 13) + 1, pw, C.byref(plan), pg, 1, po, (1 << 28) + (1 << 15), ps) == K.KICP_ERR_CAPACITY
    assert lib.kicp_plan_weights(50, 4, 5, 253, 0, None) == K.KICP_ERR_ARG
    assert lib.kicp_grid_potential_of_costmap(None, pc, pw, C.byref(plan), pg, 1, po, 24, ps) == K.KICP_ERR_ARG
    assert lib.kicp_grid_potential(None, None, None, 0, 0, pw, C.byref(plan), pg, 1, po, 24, ps) == K.KICP_ERR_ARG


def _build(tmp_path, name, extra):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I", include, "-I",
                           os.path.join(ROOT, "kinematic_icp_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "nav_host_test.cpp"), "-o", exe] + extra)
    return exe


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_nav_host_stand_alone(tmp_path, reference, flags):
    """nav_host:: in a program of its own (tests/cpp/nav_host_test.cpp), as a subprocess; the sanitizers run on this host program only.
    The path's buffer holds exactly the cells the restatement's path has - or three, to see a short buffer handled"""
    exe = _build(tmp_path, "nav_host_test", flags)
    plans = [(50, 4, 5, 253, 0), (1, 0, 1, 255, 255), (20, 0xFFFFFFFF, 1, 100, 0)]
    runs = 0
    for k, (name, (costmap, weight, goals, max_potential)) in enumerate(sorted(CASES.items())):
        want, want_stats = reference[name]
        H, W = costmap.shape
        ys, xs = np.nonzero(want != pr.UNREACHED)
        start = (int(xs[-1]), int(ys[-1])) if len(xs) else (W - 1, H - 1)
        cells = pr.path(want, costmap, weight, start)
        status = {"unreachable": 1, "clamped": 2}.get(cells, 0) if isinstance(cells, str) else 0
        cap = 3 if k % 4 == 3 else (len(cells) if status == 0 else 0)
        plan = plans[k % len(plans)]
        src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
        with open(src, "wb") as f:
            np.array([W, H, max_potential, len(goals), start[0], start[1]] + list(plan), dtype=np.uint32).tofile(f)
            np.asarray(weight, dtype=np.uint8).tofile(f), costmap.tofile(f), np.array(goals, dtype=np.uint32).tofile(f)
        out = subprocess.run([exe, src, dst, str(cap)], capture_output=True, text=True)
        assert out.returncode == 0, (out.stdout + out.stderr)[-2000:]
        raw = open(dst, "rb").read()
        assert np.array_equal(np.frombuffer(raw[:4 * W * H], dtype=np.uint32).reshape(H, W), want), name
        assert tuple(np.frombuffer(raw[4 * W * H:4 * W * H + 32], dtype=np.uint64).tolist()) == want_stats + (0,)
        rc, n = np.frombuffer(raw[4 * W * H + 32:4 * W * H + 40], dtype=np.uint32).tolist()
        assert rc == status and n == (len(cells) if status == 0 else 0), (name, rc, n)
        stored = min(n, cap)
        got = np.frombuffer(raw[4 * W * H + 40:4 * W * H + 40 + 8 * stored], dtype=np.uint32).reshape(stored, 2)
        assert status != 0 or [tuple(c) for c in got.tolist()] == cells[:stored]
        assert len(raw) == 4 * W * H + 40 + 8 * stored + 256 and np.array_equal(np.frombuffer(raw[-256:], dtype=np.uint8), pr.weights(*plan))
        runs += 1
    assert runs >= 20
