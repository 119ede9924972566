"""The restatement of include/kicp.h's text on scoring a tree of arc segments (kicp_grid_score_arc_tree, kicp_score_arc_tree_from_plan,
kicp_arc_tree_nodes, kicp_arc_tree_best) in Python floats, on top of tests/arcs_ref.py's step, pose_weight and cell_index.  Every node
is rolled from `start` on its own, through all the segments of its path: nothing is shared between nodes here, so equality with the
library also shows that continuing a prefix rolled once changes no bit."""
import numpy as np

import arcs_ref as ar

UNREACHED = ar.UNREACHED
MAX_DEPTH, MAX_NODES, MAX_T = 8, 1 << 20, 1024
INHERITED, OWN, ALIVE = 0, 1, 2  # a node's class: it ended in a segment above its own, inside its own, or took every step


def nodes(branch, steps):
    """-> (n_nodes, n_leaves, total_steps, level_offset), or the name of the rule the tree breaks: "arg" or "capacity" """
    branch, steps = [int(b) for b in branch], [int(s) for s in steps]
    if len(branch) < 1 or len(branch) != len(steps) or min(branch) < 1 or min(steps) < 1:
        return "arg"
    if len(branch) > MAX_DEPTH or sum(steps) > MAX_T:
        return "capacity"
    level, total, offsets = 1, 0, []
    for b in branch:
        level *= b
        offsets.append(total)
        total += level
    if total > MAX_NODES:
        return "capacity"
    return total, level, sum(steps), tuple(offsets)


def path_of(branch, level, index):
    """the primitives (b_1 .. b_level) of the node with in-level index `index` at `level` (1-based): repeated division"""
    path = []
    for e in range(level - 1, -1, -1):
        path.append(index % branch[e])
        index //= branch[e]
    return tuple(reversed(path))


def score_node(geom, q, potential, start, segments, footprint):
    """one trajectory: segments = [(step row, its steps), ...] -> (free_steps, cost_sum, cost_max, end_potential), the node's class"""
    pose, free, total, largest, ended_in = tuple(start), 0, 0, 0, None
    for e, (arc, n_steps) in enumerate(segments):
        for _ in range(n_steps):
            nxt = ar.step(pose, arc)
            m = ar.pose_weight(geom, q, nxt, footprint)
            if m == 0:
                ended_in = e
                break
            pose, free, total, largest = nxt, free + 1, total + m, max(largest, m)
        if ended_in is not None:
            break
    at = ar.cell_index(geom, pose[0], pose[1])
    end = int(potential[at[1]][at[0]]) if at is not None else UNREACHED
    return (free, total, largest, end), (ALIVE if ended_in is None else OWN if ended_in == len(segments) - 1 else INHERITED)


def score_tree(q, potential, cell, origin_x, origin_y, start, branch, steps, primitives, footprint, return_classes=False):
    """-> uint32 (N, 4), level-major; with return_classes also an int array (N,) of INHERITED / OWN / ALIVE"""
    branch, steps = [int(b) for b in branch], [int(s) for s in steps]
    geom = (float(cell), float(origin_x), float(origin_y), len(q[0]), len(q))
    ql, pl = np.asarray(q).tolist(), np.asarray(potential).tolist()
    fp = [(float(a), float(b)) for a, b in np.asarray(footprint, dtype=np.float64).tolist()]
    s = [float(v) for v in start]
    rows = np.asarray(primitives, dtype=np.float64).reshape(-1, 4).tolist()
    first = [sum(branch[:e]) for e in range(len(branch))]  # the row level e + 1's primitives begin at
    out, classes, count = [], [], 1
    for level in range(1, len(branch) + 1):
        count *= branch[level - 1]
        for j in range(count):
            segments = [(rows[first[e] + b], steps[e]) for e, b in enumerate(path_of(branch, level, j))]
            row, cls = score_node(geom, ql, pl, s, segments, fp)
            out.append(row), classes.append(cls)
    res = np.array(out, dtype=np.uint32).reshape(-1, 4)
    return (res, np.array(classes)) if return_classes else res


def best(results, branch, steps, w_potential=1, w_cost=0, w_blocked=0, min_free_steps=1):
    """the admissible leaf of least score, the lowest in-level index on a tie -> (leaf, path); None when none is admissible"""
    n_nodes, n_leaves, total_steps, offsets = nodes(branch, steps)
    leaves = np.asarray(results, dtype=np.uint32).reshape(n_nodes, 4)[offsets[-1]:]
    leaf = ar.arcs_best(leaves, total_steps, w_potential, w_cost, w_blocked, min_free_steps)
    return None if leaf is None else (leaf, path_of([int(b) for b in branch], len(branch), leaf))


def pinned_8x6_tree():
    """arcs_ref.pinned_8x6()'s map under a tree of branch (2, 2), steps (1, 2): both levels offer the straight step and the quarter
    turn -> (branch, steps, primitives, expected).  Level 1, one step from (0.75, 0.75) heading +x: either primitive moves to
    (1.25, 0.75), cell (2, 1), under weights of 10 - the turn ends heading +y.  Level 2, two steps each:
      straight, straight   (1.75, 0.75) lies under (3,1) (4,1) (3,2) -> 50; at (2.25, 0.75) the sample ahead is in (5, 1), impassable
      straight, turn       (1.75, 0.75) heading +y: (3,1) (3,2) (2,1) -> 30; (1.75, 1.25) heading -x: (3,2) (2,2) (3,1) -> 30
      turn, straight       (1.25, 1.25) heading +y: (2,2) (2,3) (1,2) -> 20; (1.25, 1.75): (2,3) (2,4) (1,3) -> 10
      turn, turn           (1.25, 1.25) heading -x: (2,2) (1,2) (2,1) -> 20; (0.75, 1.25) heading -y: (1,2) (1,1) (2,2) -> 20
    with the potential 100 y + x at the last free pose's cell."""
    straight, turn = [0.5, 0.0, 1.0, 0.0], [0.5, 0.0, 0.0, 1.0]
    expected = np.array([[1, 10, 10, 102], [1, 10, 10, 102], [2, 60, 50, 103], [3, 70, 30, 203], [3, 40, 20, 302], [3, 50, 20, 201]], dtype=np.uint32)
    return (2, 2), (1, 2), np.array([straight, turn, straight, turn]), expected


FUZZ_SEED = 77  # of the primitives and the start of "fuzz_8_6_5" below; test_gpu_arc_tree.py asserts what it was chosen for


def small_cases():
    """name -> (q, goals, max_potential, cell, origin_x, origin_y, start, branch, steps, primitives, footprint).  q is a costmap under
    IDENTITY weights (tests/potential_ref.py); the potential is the field of `goals` over it, clamped at max_potential.  The smallest
    shapes at which the kernel's mapping - a wave per node, four nodes per workgroup, a node's parent and primitive by division, lanes
    striding the samples, a launch per level - can go wrong."""
    import potential_ref as pr
    cases = {}
    rng = np.random.Generator(np.random.PCG64(11))
    box53 = ar.footprint_box(-0.2, 0.2, -0.1, 0.1, 0.1)  # 5 x 3 samples
    far = pr.MAX_POTENTIAL
    for n in (1, 3, 4, 5, 257):  # the workgroup's edges and a partial last one: at the last level, and at level 1 of a tree of depth 1
        q = pr.random_costmap(33, 31, 60 + n, 0.1)
        start, at = ar.open_start(q, 0.25, -1.0, -2.0, rng)
        cases["last_level_%d" % n] = (q, [at], far, 0.25, -1.0, -2.0, start, (1, n), (2, 6), ar.random_arcs(rng, 1 + n, step=0.2), box53)
        cases["depth_1_of_%d" % n] = (q, [at], far, 0.25, -1.0, -2.0, start, (n,), (8,), ar.random_arcs(rng, n), box53)
    for n_samples in (1, 63, 64, 65, 130):  # the lane stride's edges
        q = pr.random_costmap(33, 31, 80 + n_samples, 0.03)
        start, at = ar.open_start(q, 0.25, -1.0, -2.0, rng)
        cases["samples_%d" % n_samples] = (q, [at], far, 0.25, -1.0, -2.0, start, (3, 4), (3, 3), ar.random_arcs(rng, 7), rng.uniform(-0.3, 0.3, (n_samples, 2)))
    q = pr.random_costmap(33, 31, 7, 0.1)
    start, at = ar.open_start(q, 0.25, -1.0, -2.0, rng)
    cases["steps_1_1"] = (q, [at], far, 0.25, -1.0, -2.0, start, (3, 3), (1, 1), ar.random_arcs(rng, 6), box53)
    q = pr.random_costmap(33, 31, 8, 0.05)
    start, at = ar.open_start(q, 0.25, -1.0, -2.0, rng)
    cases["depth_8"] = (q, [at], far, 0.25, -1.0, -2.0, start, (2,) * 8, (1,) * 8, ar.random_arcs(rng, 16, step=0.2), box53)
    # arcs_ref's wall at x in [5.0, 5.25): the parents collide at their first step, at their last step and never; under each, a child
    # that would collide at its own first step, a slow one and one that backs off; and a third level under those
    wall = np.full((31, 33), 7, dtype=np.uint8)
    wall[:, 20] = 0
    three = np.array([[0.0, 0.0], [0.25, 0.0], [-0.25, 0.0]])
    rows = np.array([[2.25, 0.0, 1.0, 0.0], [0.45, 0.0, 1.0, 0.0], [0.1, 0.0, 1.0, 0.0],
                     [2.25, 0.0, 1.0, 0.0], [0.1, 0.0, 1.0, 0.0], [-0.3, 0.0, 1.0, 0.0],
                     [0.2, 0.0, 1.0, 0.0], [1.0, 0.0, 1.0, 0.0]])
    cases["wall"] = (wall, [(0, 0)], far, 0.25, 0.0, 0.0, (2.625, 3.875, 1.0, 0.0), (3, 3, 2), (5, 3, 2), rows, three)
    field = np.full((31, 33), 5, dtype=np.uint8)
    mid = ar.centre(0.25, -1.0, -2.0, 16, 15)
    nan, inf = float("nan"), float("inf")
    bad = np.array([[0.1, 0.0, 1.0, 0.0], [-0.1, 0.05, 1.0, 0.0],
                    [nan, 0.0, 1.0, 0.0], [0.1, inf, 1.0, 0.0], [0.1, 0.0, -inf, 0.0], [0.1, 0.0, 1.0, nan], [0.1, 0.0, 1.0, 0.0]])
    cases["level_2_not_finite"] = (field, [(16, 15)], far, 0.25, -1.0, -2.0, mid + (1.0, 0.0), (2, 5), (3, 4), bad, box53)
    fp = box53.copy()
    fp[7] = (nan, 0.0)
    cases["footprint_nan"] = (field, [(16, 15)], far, 0.25, -1.0, -2.0, mid + (1.0, 0.0), (2, 2), (2, 2), bad[[0, 1, 0, 1]], fp)
    cases["start_outside"] = (field, [(16, 15)], far, 0.25, -1.0, -2.0, (-3.0, -4.0, 1.0, 0.0), (2, 2), (3, 2),
                              np.array([[0.1, 0.0, 1.0, 0.0], [2.5, 2.5, 1.0, 0.0], [0.1, 0.0, 1.0, 0.0], [-0.5, -0.5, 1.0, 0.0]]), box53)
    sides = np.array([[0.5, 0.0, 1.0, 0.0], [-0.5, 0.0, 1.0, 0.0], [0.0, 0.5, 1.0, 0.0], [0.0, -0.5, 1.0, 0.0]])
    cases["four_sides"] = (field, [(16, 15)], far, 0.25, -1.0, -2.0, mid + (1.0, 0.0), (4, 4), (3, 30), np.concatenate([sides, sides]), box53)
    # from the goal's cell (2, 2) to (4, 3), then one jump into the ring no path enters, (18, 16), and one to the far corner (38, 34), beyond the clamp
    one = np.array([[0.0, 0.0]])
    cases["unreached_and_clamped"] = (pr.enclosed(), [(2, 2)], 300, 0.25, 0.0, 0.0, (0.625, 0.625, 1.0, 0.0), (1, 2), (1, 1),
                                      np.array([[0.5, 0.25, 1.0, 0.0], [3.5, 3.25, 1.0, 0.0], [8.5, 7.75, 1.0, 0.0]]), one)
    q = pr.random_costmap(70, 50, 9, 0.1)
    frng = np.random.Generator(np.random.PCG64(FUZZ_SEED))
    start, at = ar.open_start(q, 0.25, -1.0, -2.0, frng)
    cases["fuzz_8_6_5"] = (q, [at], far, 0.25, -1.0, -2.0, start, (8, 6, 5), (5, 4, 3), ar.random_arcs(frng, 19, step=0.3), box53)
    return cases


def check_case(name, res, classes, branch, steps, pot):
    """what each case is there for shows in its result (shared by the host and the GPU suite); classes: the restatement's"""
    n_nodes, n_leaves, total, offsets = nodes(branch, steps)
    assert res.shape == (n_nodes, 4) and (res[:, 0] <= total).all()
    levels = [res[o:o + n] for o, n in zip(offsets, [int(np.prod(branch[:e + 1])) for e in range(len(branch))])]
    if name == "wall":
        l1, l2, l3 = levels
        assert l1[:, 0].tolist() == [0, 4, 5] and l1[0].tolist() == [0, 0, 0, int(pot[15, 10])]  # at step 1, at step L_1, never
        assert np.array_equal(l2[:3], np.repeat(l1[:1], 3, axis=0)) and np.array_equal(l2[3:6], np.repeat(l1[1:2], 3, axis=0))  # the children inherit
        assert l2[6].tolist() == l1[2].tolist() and classes[offsets[1] + 6] == OWN  # collides at its own first step: the parent's total, and its words
        assert l2[7:, 0].tolist() == [8, 8] and np.array_equal(l3[12:14], np.repeat(l2[6:7], 2, axis=0))  # and its children inherit those
        assert l3[14:, 0].tolist() == [10, 9, 10, 10] and (classes[:offsets[1]] == [OWN, OWN, ALIVE]).all()
    if name == "level_2_not_finite":
        assert levels[0][:, 0].tolist() == [3, 3] and levels[1][:, 0].tolist() == [3, 3, 3, 3, 7] * 2
        assert np.array_equal(levels[1][:4], np.repeat(levels[0][:1], 4, axis=0))
    if name == "footprint_nan":
        assert (res[:, 0] == 0).all() and (classes[offsets[1]:] == INHERITED).all()
    if name == "start_outside":
        assert levels[0].tolist() == [[0, 0, 0, UNREACHED], [3, 15, 5, int(pot[22, 22])]] and levels[1][:2].tolist() == [[0, 0, 0, UNREACHED]] * 2
        assert levels[1][2:, 0].tolist() == [5, 5]
    if name == "four_sides":
        assert (levels[0][:, 0] == 3).all() and (levels[1][:, 0] > 3).all() and (levels[1][:, 0] < total).all() and (res[:, 3] != UNREACHED).all()
    if name == "unreached_and_clamped":
        assert res.tolist() == [[1, 7, 7, int(pot[3, 4])], [2, 14, 7, UNREACHED], [2, 14, 7, 300]]
    if name == "depth_8":
        assert n_nodes == 510 and n_leaves == 256 and (levels[7][:, 0] == 8).any()
    if name.startswith("depth_1_of_") or name.startswith("last_level_"):
        assert n_leaves == int(name.rsplit("_", 1)[1])
