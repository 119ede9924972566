"""Inputs shared by the tests of the class ROUGH (tests/test_elev_rough_cases.py proves what each is for, tests/test_elev_rough_host.py
runs the host code over them, tests/test_gpu_elev_rough.py the kernels): exact planes and one raised cell - Q by hand -, the strict
comparison at equality, a product beyond 64 bits, fits of three cells, lines and min_cells, the gate and Szz, tile borders and the
halo, the slope suite's random columns and the columns of its drive.
A CASE is (name, columns uint64 [H, W], (S, H), slope = (L, K, min_cells, rise, run), rough = (num, den), rectangles); the expected
results come from tests/elev_rough_ref.py, once (expected())."""
import functools

import numpy as np

import elev_cases as ec
import elev_ref as er
import elev_rough_ref as rr
import elev_slope_cases as sc

NO_STEP = sc.NO_STEP
NO_SLOPE = (65535, 1)  # rise, run under which no case below is SLOPE: the verdict is ROUGH's alone
ANY = (0, 1)           # num, den: every residual above zero is ROUGH


# ---- an exact plane, and one cell of it raised --------------------------------------------------------------------------------------
PLANE_SIDE, BUMP_CELL, BUMP = 9, (4, 4), 3  # (x, y)
# The middle cell at L = 1, by hand.  The window is full: n = 9, Sx = Sy = Sxy = 0, Sxx = Syy = 6.  The middle cell lies 3 over the plane
# z = dx + 2 dy, so z = dx + 2 dy - 3 for the eight neighbours and 0 for itself: Sz = -24, Sxz = sum dx^2 = 6, Syz = 2 sum dy^2 = 12,
# Szz = sum (dx + 2 dy)^2 - 6 sum (dx + 2 dy) + 8 * 9 = (6 + 24) + 72 = 102.  D = 6 * 6 * 9 = 324, Da = 6 * 54 = 324, Db = 6 * 12 * 9 = 648,
# Dc = 6 * 6 * (-24) = -864, Q = 324 * 102 - 324 * 6 - 648 * 12 - 864 * 24 = 2 592.  (The fitted plane is dx + 2 dy - 8 / 3: eight
# residuals of -1 / 3 and one of 8 / 3, a sum of squares of 8 = Q / D.)  Q den == num n D at num / den = 2 592 / 2 916 = 8 / 9.
BUMP_FIT = (324, 324, 648, 2592, 9)
BUMP_EQUAL = (8, 9)


def plane_layer(bump=0):
    y, x = np.mgrid[0:PLANE_SIDE, 0:PLANE_SIDE]
    g = 20 + x + 2 * y
    g[BUMP_CELL[1], BUMP_CELL[0]] += bump
    return sc.from_grounds(g)


# ---- a product beyond 64 bits ----------------------------------------------------------------------------------------------------------
WIDE_SIDE, WIDE_CELL, WIDE_SLOPE = 25, (12, 12), (8, 63, 289) + NO_SLOPE


def checkerboard():
    y, x = np.mgrid[0:WIDE_SIDE, 0:WIDE_SIDE]
    return sc.from_grounds(np.where((x + y) % 2 == 0, 0, 63))


@functools.lru_cache(maxsize=None)
def wide_rough():
    """(num, den) for the checkerboard, num = 65535 and den the largest for which at WIDE_CELL the low 64 bits of Q den fall below
    num n D while Q den itself lies above it: a left side wrapped to 64 bits gives the other verdict"""
    c = rr.classify(checkerboard(), *NO_STEP, WIDE_SLOPE, (0, 1))
    x, y = WIDE_CELL
    q, right = int(c.Q[y, x]), 65535 * int(c.sums["n"][y, x]) * int(c.D[y, x])
    for den in range(65535, 0, -1):
        if q * den >= 1 << 64 and (q * den) % (1 << 64) <= right < q * den:
            return 65535, den
    raise AssertionError("no such den")


# ---- three cells, lines, min_cells ----------------------------------------------------------------------------------------------------
def three_cells():
    """5 x 5 cells, three known and not on one line, at any grounds: a plane goes through them, Q = 0"""
    g = np.full((5, 5), 255, dtype=np.int64)
    g[2, 2], g[1, 3], g[3, 3] = 30, 41, 17
    return sc.from_grounds(g)


# ---- the gate and Szz -------------------------------------------------------------------------------------------------------------------
GATE_MID = (2, 2)  # sc.gate_layer(20, 27) at K = 6: eight level cells fit, Q = 0; the ninth, 7 over them, must stay out of Szz too


# ---- tile borders ---------------------------------------------------------------------------------------------------------------------
BORDER_SIDE = 34
# (bump cell, witness cell), (x, y) each: level ground but for the bumps; the witness lies beside the bump on the other side of a tile
# border (16, 32; the tiles start at the rectangle's corner), in both directions across each border, and across a tile corner
BORDER_PAIRS = [((16, 8), (15, 8)), ((15, 24), (16, 24)), ((8, 16), (8, 15)), ((24, 15), (24, 16)), ((32, 4), (31, 4)), ((31, 20), (32, 20)), ((4, 32), (4, 31)),
                ((20, 31), (20, 32)), ((16, 16), (15, 15)), ((31, 31), (32, 32))]


def border_layer(without=None):
    g = np.full((BORDER_SIDE, BORDER_SIDE), 10, dtype=np.int64)
    for bump, _ in BORDER_PAIRS:
        if bump != without:
            g[bump[1], bump[0]] = 15
    return sc.from_grounds(g)


# sc.tilted_square's noise leaves a mean squared residual of 0.05 .. 0.4 slab^2 at L = 1 and of 0.24 .. 0.37 at L = 8: limits inside
SQUARE_ROUGH = {1: (1, 4), 8: (3, 10)}

# ---- random columns, and the drive ----------------------------------------------------------------------------------------------------
RANDOM_ROUGH = [(1, 2), (512, 1024), ANY, (65535, 1), (1, 65535)]  # beside sc.RANDOM_CONFIGS, in its order
DRIVE_ROUGH = (512, 1024)  # half a slab^2: an r.m.s. residual of 4.4 cm on the drive's 0.0625 m slabs


def small_cases():
    """every hand-made case: (name, columns, (S, H), slope, rough, rectangles)"""
    cases = [("plane_L%d" % L, plane_layer(), NO_STEP, (L, 63, 3) + NO_SLOPE, ANY, [None, (6, 5, 3, 4)]) for L in (1, 2, 8)]
    cases += [("bump_L1", plane_layer(BUMP), NO_STEP, (1, 63, 3) + NO_SLOPE, ANY, [None, (BUMP_CELL[0], BUMP_CELL[1], 1, 1)]),
              ("bump_equal", plane_layer(BUMP), NO_STEP, (1, 63, 3) + NO_SLOPE, BUMP_EQUAL, [None]),
              ("bump_below", plane_layer(BUMP), NO_STEP, (1, 63, 3) + NO_SLOPE, (BUMP_EQUAL[0] - 1, BUMP_EQUAL[1]), [None])]
    cases += [("checkerboard", checkerboard(), NO_STEP, WIDE_SLOPE, wide_rough(), [None, (WIDE_CELL[0], WIDE_CELL[1], 1, 1), (9, 3, 16, 22)]),
              ("checkerboard_never", checkerboard(), NO_STEP, WIDE_SLOPE, (65535, 1), [None]),
              ("split", sc.wide_layer(), NO_STEP, WIDE_SLOPE, (65535, 65535), [None, (sc.WIDE_SPLIT, 8, 1, 9)])]
    cases.append(("three_cells", three_cells(), NO_STEP, (1, 63, 3) + NO_SLOPE, ANY, [None]))
    tilt, diagonal = sc.min_cells_layer()
    cases += [("min_cells_met", tilt, NO_STEP, (2, 63, 7) + NO_SLOPE, ANY, [None]), ("min_cells_missed", tilt, NO_STEP, (2, 63, 8) + NO_SLOPE, ANY, [None]),
              ("on_one_line", diagonal, NO_STEP, (2, 63, 3) + NO_SLOPE, ANY, [None])]
    cases += [("gate_out", sc.gate_layer(20, 27), NO_STEP, (1, 6, 3) + NO_SLOPE, ANY, [None]), ("gate_in", sc.gate_layer(20, 26), NO_STEP, (1, 6, 3) + NO_SLOPE, ANY, [None])]
    # geometry: every rectangle's tiles overhang the layer or the rectangle
    overhang = {"one_cell": [None], "one_row": [None, (33, 0, 7, 1), (5, 0, 17, 1)], "one_column": [None, (0, 33, 1, 7), (0, 5, 1, 17)]}
    cases += [(name, columns, NO_STEP, (4, 63, 3) + NO_SLOPE, ANY, overhang[name]) for name, columns in sc.collinear_layers()]
    for side in sc.SQUARE_SIDES:
        for slope in sc.SQUARE_SLOPES:
            rects = [None] + ([(side - 9, 3, 9, side - 3), (15, 15, 2, 2)] if side > 16 else [(side - 1, side - 1, 1, 1), (2, 1, side - 2, side - 1)])
            cases.append(("square%d_L%d" % (side, slope[0]), sc.tilted_square(side, 100 + side), (2, 8), slope, SQUARE_ROUGH[slope[0]], rects))
    cases.append(("borders", border_layer(), NO_STEP, (1, 63, 3) + NO_SLOPE, ANY, [None, (3, 5, 31, 29), (15, 15, 19, 19)]))
    columns, slope = sc.wrap_layer()
    cases.append(("wrap", columns, NO_STEP, slope[:3] + NO_SLOPE, ANY, [None, (sc.WRAP_CELL[0], sc.WRAP_CELL[1], 1, 1), (17, 0, 3, 12)]))
    return cases


def random_cases():
    return [("random_%s_%d" % (kind, k), ec.random_columns(kind), params, slope, RANDOM_ROUGH[k], ec.RECTS) for kind in ("dense", "sparse", "zero")
            for k, (params, slope) in enumerate(sc.RANDOM_CONFIGS)]


def all_cases():
    return small_cases() + random_cases()


def radius_cases():
    """sc.radius_cases() with the squares' limit at L = 1 for ROUGH"""
    return [(name, columns, params, slope, (1, 4), rects) for name, columns, params, slope, rects in sc.radius_cases()]


_expected = {}


def expected(case):
    """the restatement's result for a case's full layer - computed once per case and shared; nobody changes it"""
    name, columns, (S, H), slope, rough, _ = case
    if name not in _expected:
        _expected[name] = rr.classify(columns, S, H, slope, rough)
    return _expected[name]


def check_result(case, rect, got, got_ground=None, got_fit=None, got_counts=None):
    """a result of one rectangle of a case against the restatement: np.array_equal and == throughout"""
    name, columns = case[0], case[1]
    want = expected(case)
    r = rect or (0, 0, columns.shape[1], columns.shape[0])
    assert got.dtype == np.int8 and got.shape == (r[3], r[2]), (name, rect)
    assert np.array_equal(got, er.restrict(want.classes, r)), (name, rect)
    if got_ground is not None:
        assert got_ground.dtype == np.uint8 and np.array_equal(got_ground, er.restrict(want.ground, r)), (name, rect)
    if got_fit is not None:
        assert got_fit.dtype == np.int64 and got_fit.shape == (r[3], r[2], 5) and np.array_equal(got_fit, er.restrict(want.fit, r)), (name, rect)
    if got_counts is not None:
        assert got_counts == rr.counts(want, r), (name, rect, got_counts, rr.counts(want, r))
