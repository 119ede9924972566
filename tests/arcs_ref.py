"""The restatement of include/kicp.h's text on scoring a fan of arc trajectories (kicp_grid_score_arcs, kicp_score_arcs_from_plan,
kicp_arc_steps, kicp_footprint_box, kicp_arcs_best, kicp_plan_q) in Python floats and `math`, one IEEE operation per expression: a
Python float is an fp64 and + - * / round each on their own, so what this file computes is what the header says, bit for bit.  No
numpy arithmetic on the values that matter; numpy only carries the arrays."""
import math

import numpy as np

UNREACHED = 0xFFFFFFFF
MASK64 = (1 << 64) - 1


def step(pose, arc):
    """pose_t from pose_{t-1} = (x, y, c, s) and the arc's step (dx, dy, dc, ds)"""
    x, y, c, s = pose
    dx, dy, dc, ds = arc
    a = c * dx
    b = s * dy
    nx = x + (a - b)
    a = s * dx
    b = c * dy
    ny = y + (a + b)
    a = c * dc
    b = s * ds
    nc = a - b
    a = s * dc
    b = c * ds
    ns = a + b
    return nx, ny, nc, ns


def cell_of(w, origin, cell):
    """floor((w - origin) / cell) as a Python int, None when it is not finite"""
    d = w - origin
    v = d / cell
    return math.floor(v) if math.isfinite(v) else None


def cell_index(geom, wx, wy):
    """(cx, cy) of a world point inside the grid, else None; geom = (cell, origin_x, origin_y, width, height)"""
    cell, ox, oy, width, height = geom
    if not (math.isfinite(wx) and math.isfinite(wy)):
        return None
    cx, cy = cell_of(wx, ox, cell), cell_of(wy, oy, cell)
    if cx is None or cy is None or not (0 <= cx < width and 0 <= cy < height):
        return None
    return cx, cy


def pose_weight(geom, q, pose, footprint):
    """0 when the pose collides, else the largest weight under the footprint's samples"""
    x, y, c, s = pose
    largest = 0
    for fx, fy in footprint:
        a = c * fx
        b = s * fy
        wx = x + (a - b)
        a = s * fx
        b = c * fy
        wy = y + (a + b)
        at = cell_index(geom, wx, wy)
        w = int(q[at[1]][at[0]]) if at is not None else 0
        if w == 0:
            return 0
        largest = max(largest, w)
    return largest


def score_arc(geom, q, potential, start, arc, n_steps, footprint):
    pose, free, total, largest = tuple(start), 0, 0, 0
    for _ in range(n_steps):
        nxt = step(pose, arc)
        m = pose_weight(geom, q, nxt, footprint)
        if m == 0:
            break
        pose, free, total, largest = nxt, free + 1, total + m, max(largest, m)
    at = cell_index(geom, pose[0], pose[1])
    return free, total, largest, int(potential[at[1]][at[0]]) if at is not None else UNREACHED


def score_arcs(q, potential, cell, origin_x, origin_y, start, arcs, n_steps, footprint):
    """-> uint32 (K, 4): free_steps, cost_sum, cost_max, end_potential"""
    geom = (float(cell), float(origin_x), float(origin_y), len(q[0]), len(q))
    ql, pl = np.asarray(q).tolist(), np.asarray(potential).tolist()
    fp = [(float(a), float(b)) for a, b in np.asarray(footprint, dtype=np.float64).tolist()]
    s = [float(v) for v in start]
    return np.array([score_arc(geom, ql, pl, s, [float(v) for v in arc], n_steps, fp) for arc in np.asarray(arcs, dtype=np.float64).tolist()], dtype=np.uint32).reshape(-1, 4)


def arc_steps(v, omega, dt):
    """-> float64 (K, 4): dx, dy, dc, ds; the branch stands where the reference adds an epsilon"""
    out = []
    for vk, wk in zip(np.asarray(v, dtype=np.float64).tolist(), np.asarray(omega, dtype=np.float64).tolist()):
        d = vk * dt
        theta = wk * dt
        sn, cs = math.sin(theta), math.cos(theta)
        if abs(theta) < 1e-9:
            dx, dy = d, 0.0
        else:
            a = d * sn
            dx = a / theta
            a = 1.0 - cs
            a = d * a
            dy = a / theta
        out.append((dx, dy, cs, sn))
    return np.array(out, dtype=np.float64).reshape(-1, 4)


def axis(lo, hi, spacing):
    d = hi - lo
    n = math.ceil(d / spacing) + 1
    if n == 1:
        return [lo]
    out = []
    for i in range(n):
        a = d * float(i)
        a = a / float(n - 1)
        out.append(lo + a)
    return out


def footprint_box(x_min, x_max, y_min, y_max, spacing):
    """-> float64 (nx * ny, 2), x running fastest"""
    xs, ys = axis(x_min, x_max, spacing), axis(y_min, y_max, spacing)
    return np.array([(x, y) for y in ys for x in xs], dtype=np.float64).reshape(-1, 2)


def arcs_best(results, n_steps, w_potential=1, w_cost=0, w_blocked=0, min_free_steps=1):
    """the admissible arc of least score, lowest index on a tie; None when none is admissible"""
    best, least = None, None
    for k, (free, total, _, end) in enumerate(np.asarray(results, dtype=np.uint32).tolist()):
        if free < min_free_steps or end == UNREACHED:
            continue
        score = (w_potential * end + w_cost * total + w_blocked * max(n_steps - free, 0)) & MASK64
        if best is None or score < least:
            best, least = k, score
    return best


def pinned_8x6():
    """8 x 6 cells of 0.5 m from the origin, a three-sample footprint, a straight arc that collides at step 3 and a quarter-turn arc
    that comes back to where it started -> (q, potential, cell, start, arcs, n_steps, footprint, expected)"""
    q = np.full((6, 8), 10, dtype=np.uint8)
    q[1, 4], q[1, 5], q[2, 3], q[2, 1] = 50, 0, 30, 20
    potential = (100 * np.arange(6)[:, None] + np.arange(8)[None, :]).astype(np.uint32)
    start = (0.75, 0.75, 1.0, 0.0)
    arcs = np.array([[0.5, 0.0, 1.0, 0.0], [0.5, 0.0, 0.0, 1.0]])
    footprint = np.array([[0.0, 0.0], [0.5, 0.0], [0.0, 0.5]])
    # straight: poses at x = 1.25, 1.75, 2.25; under the footprint (2,1) (3,1) (2,2) -> 10, then (3,1) (4,1) (3,2) -> 50, then (5,1) is
    # impassable: two free steps, the end is the cell (3, 1).  turning: four quarter turns round (1,1) (2,1) (2,2) (1,2), the cell
    # (1, 2) weighs 20 and lies under the footprint at the poses 2, 3 and 4; the end is the start's cell (1, 1).
    expected = np.array([[2, 60, 50, 103], [4, 70, 20, 101]], dtype=np.uint32)
    return q, potential, 0.5, start, arcs, 4, footprint, expected


def random_arcs(rng, n, step=0.3, turn=0.3):
    """n arcs: dx within +-step, a little dy, a yaw within +-turn a step"""
    theta = rng.uniform(-turn, turn, n)
    return np.stack([rng.uniform(-step, step, n), rng.uniform(-0.05, 0.05, n), np.cos(theta), np.sin(theta)], axis=1)


def centre(cell, origin_x, origin_y, cx, cy):
    return origin_x + (cx + 0.5) * cell, origin_y + (cy + 0.5) * cell


def open_start(q, cell, origin_x, origin_y, rng):
    """a start in the middle of a passable cell whose eight neighbours are passable too, with a random heading"""
    ok = np.argwhere(q[1:-1, 1:-1] > 0)
    ok = [(x + 1, y + 1) for y, x in ok.tolist() if (q[y:y + 3, x:x + 3] > 0).all()]
    cx, cy = ok[int(rng.integers(len(ok)))]
    yaw = float(rng.uniform(-math.pi, math.pi))
    return centre(cell, origin_x, origin_y, cx, cy) + (math.cos(yaw), math.sin(yaw)), (cx, cy)


def small_cases():
    """name -> (q, goals, max_potential, cell, origin_x, origin_y, start, arcs, n_steps, footprint).  q is a costmap under IDENTITY
    weights (tests/potential_ref.py); the potential is the field of `goals` over it, clamped at max_potential.  The smallest shapes at
    which the kernel's mapping - a wave per arc, four arcs per workgroup, lanes striding the samples - can go wrong."""
    import potential_ref as pr
    cases = {}
    rng = np.random.Generator(np.random.PCG64(5))
    box53 = footprint_box(-0.2, 0.2, -0.1, 0.1, 0.1)  # 5 x 3 samples
    assert box53.shape == (15, 2)
    far = pr.MAX_POTENTIAL
    for n_samples in (1, 63, 64, 65, 130):  # the lane stride's edges
        q = pr.random_costmap(33, 31, n_samples, 0.03)
        start, at = open_start(q, 0.25, -1.0, -2.0, rng)
        cases["samples_%d" % n_samples] = (q, [at], far, 0.25, -1.0, -2.0, start, random_arcs(rng, 6), 6, rng.uniform(-0.3, 0.3, (n_samples, 2)))
    for n_arcs in (1, 3, 4, 5, 257):  # the workgroup's edges and a partial last one
        q = pr.random_costmap(33, 31, 40 + n_arcs, 0.1)
        start, at = open_start(q, 0.25, -1.0, -2.0, rng)
        cases["arcs_%d" % n_arcs] = (q, [at], far, 0.25, -1.0, -2.0, start, random_arcs(rng, n_arcs), 8, box53)
    # a wall at x in [5.0, 5.25): collide at step 1, at step T, never; and T = 1
    wall = np.full((31, 33), 7, dtype=np.uint8)
    wall[:, 20] = 0
    three = np.array([[0.0, 0.0], [0.25, 0.0], [-0.25, 0.0]])
    ahead = np.array([[2.25, 0.0, 1.0, 0.0], [0.45, 0.0, 1.0, 0.0], [0.1, 0.0, 1.0, 0.0]])
    cases["wall_steps_5"] = (wall, [(0, 0)], far, 0.25, 0.0, 0.0, (2.625, 3.875, 1.0, 0.0), ahead, 5, three)
    cases["wall_steps_1"] = (wall, [(0, 0)], far, 0.25, 0.0, 0.0, (2.625, 3.875, 1.0, 0.0), ahead, 1, three)
    one = np.array([[0.0, 0.0]])
    cases["grid_1x1"] = (np.full((1, 1), 9, dtype=np.uint8), [(0, 0)], far, 1.0, 0.0, 0.0, (0.5, 0.5, 1.0, 0.0),
                         np.array([[0.1, 0.0, 1.0, 0.0], [0.3, 0.0, 1.0, 0.0], [-0.3, 0.0, 1.0, 0.0], [0.0, 0.0, math.cos(1.0), math.sin(1.0)]]), 3, one)
    field = np.full((31, 33), 5, dtype=np.uint8)
    mid = centre(0.25, -1.0, -2.0, 16, 15)
    sides = np.array([[0.5, 0.0, 1.0, 0.0], [-0.5, 0.0, 1.0, 0.0], [0.0, 0.5, 1.0, 0.0], [0.0, -0.5, 1.0, 0.0]])
    cases["four_sides"] = (field, [(16, 15)], far, 0.25, -1.0, -2.0, mid + (1.0, 0.0), sides, 30, box53)  # -x and -y give a negative floor
    cases["start_outside"] = (field, [(16, 15)], far, 0.25, -1.0, -2.0, (-3.0, -4.0, 1.0, 0.0), np.array([[0.1, 0.0, 1.0, 0.0], [2.5, 2.5, 1.0, 0.0]]), 3, box53)
    block = field.copy()
    block[15, 20:22] = 0
    long_box = footprint_box(-0.2, 1.2, -0.1, 0.1, 0.1)  # 15 x 3, the long side ahead
    cases["spin_in_place"] = (block, [(16, 15)], far, 0.25, -1.0, -2.0, mid + (0.0, 1.0), np.array([[0.0, 0.0, math.cos(-0.2), math.sin(-0.2)]]), 12, long_box)
    nan, inf = float("nan"), float("inf")
    bad = np.array([[nan, 0.0, 1.0, 0.0], [0.1, inf, 1.0, 0.0], [0.1, 0.0, -inf, 0.0], [0.1, 0.0, 1.0, nan], [0.1, 0.0, 1.0, 0.0]])
    cases["arcs_not_finite"] = (field, [(16, 15)], far, 0.25, -1.0, -2.0, mid + (1.0, 0.0), bad, 4, box53)
    for name, sample in (("nan", (nan, 0.0)), ("plus_inf", (0.0, inf)), ("minus_inf", (-inf, 0.0))):
        fp = box53.copy()
        fp[7] = sample
        cases["footprint_" + name] = (field, [(16, 15)], far, 0.25, -1.0, -2.0, mid + (1.0, 0.0), bad[3:], 4, fp)
    # (2.0 - 0.0) / 0.5 is exactly 4: the sample lies in cell 4, which is impassable; and x = 0.0 lies in cell 0
    exact = np.full((6, 8), 3, dtype=np.uint8)
    exact[1, 4] = 0
    cases["exact_integer"] = (exact, [(0, 0)], far, 0.5, 0.0, 0.0, (1.0, 0.75, 1.0, 0.0), np.array([[0.0, 0.0, 1.0, 0.0], [-0.5, 0.0, 1.0, 0.0]]), 4,
                              np.array([[0.0, 0.0], [1.0, 0.0]]))
    # one jump from the goal's cell (2, 2) into the ring no path enters, (18, 16), and one to the far corner (38, 34), beyond the clamp
    cases["unreached_and_clamped"] = (pr.enclosed(), [(2, 2)], 300, 0.25, 0.0, 0.0, (0.625, 0.625, 1.0, 0.0), np.array([[4.0, 3.5, 1.0, 0.0], [9.0, 8.0, 1.0, 0.0]]), 1, one)
    q = pr.random_costmap(70, 50, 9, 0.3)
    start, at = open_start(q, 0.25, -1.0, -2.0, rng)
    cases["fuzz_2000"] = (q, [at], far, 0.25, -1.0, -2.0, start, random_arcs(rng, 2000), 24, box53)
    q = pr.random_costmap(70, 50, 10, 0.04)
    start, at = open_start(q, 0.25, -1.0, -2.0, rng)
    cases["fuzz_sparse_500"] = (q, [at], far, 0.25, -1.0, -2.0, start, random_arcs(rng, 500), 24, box53)
    return cases
