"""Inputs shared by the slope limit's tests (tests/test_elev_slope_cases.py proves what each is for, tests/test_elev_slope_host.py runs
the host code over them, tests/test_gpu_elev_slope.py the kernels): hand-made layers of grounds - tile borders and the halo, the gate,
min_cells, the comparison, the widths of the integers -, tests/elev_cases.py's random columns and the columns of its drive.
A CASE is (name, columns uint64 [H, W], (S, H), slope = (L, K, min_cells, rise, run), rectangles); the expected results come from
tests/elev_slope_ref.py, once (expected())."""
import functools

import numpy as np

import elev_cases as ec
import elev_ref as er
import elev_slope_ref as sr

U64 = np.uint64
NO_STEP = (62, 63)  # S, H under which columns of one bit are never BODY or STEP: the verdict is the slope's alone


def from_grounds(grounds):
    """columns of one bit each: bit g where grounds is 0 .. 63, empty where it is 255 (or negative)"""
    g = np.asarray(grounds, dtype=np.int64)
    ok = (g >= 0) & (g <= 63)
    return np.where(ok, U64(1) << np.where(ok, g, 0).astype(U64), U64(0)).astype(U64)


# ---- tile borders and the halo ------------------------------------------------------------------------------------------------------
def collinear_layers():
    """1 x 1, 1 x 40 and 40 x 1 cells (height x width), the grounds rising along the line: every fit set is collinear, D = 0"""
    line = np.arange(40) % 30
    return [("one_cell", from_grounds([[5]])), ("one_row", from_grounds(line[None, :])), ("one_column", from_grounds(line[:, None]))]


def tilted_square(side, seed):
    """a side x side layer: a plane of about 0.4 slabs per cell in x and 0.7 in y with a slab of noise, four cells in five known - steeper
    than 4 / 5 for some cells and not for others, on both sides of every tile border (16, 32)"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:side, 0:side]
    g = np.floor(0.4 * x + 0.7 * y + rng.uniform(0.0, 1.6, (side, side))).astype(np.int64)
    g[rng.random((side, side)) < 0.2] = 255
    return from_grounds(g)


SQUARE_SIDES = (15, 16, 17, 31, 32, 33)
SQUARE_SLOPES = ((1, 2, 5, 4, 5), (8, 63, 12, 4, 5))  # L = 1 and L = 8

WRAP_W, WRAP_H, WRAP_CELL = 20, 12, (19, 5)  # (x, y): the last cell of row 5


def wrap_layer():
    """A level patch of ground 10 at the right border of a 20 x 12 layer around WRAP_CELL (L = 3: x 16 .. 19, y 2 .. 8), and ground 12 in
    the first three cells of the rows 3 .. 9: a halo that runs past a row's end, or wraps into the next row, reads those as the
    cells to the right of the patch - a tilt.  rise = 0: any tilt is SLOPE."""
    g = np.full((WRAP_H, WRAP_W), 255, dtype=np.int64)
    g[2:9, 16:20] = 10
    g[3:10, 0:3] = 12
    return from_grounds(g), (3, 6, 5, 0, 1)


def wrapped_view(columns, L):
    """the layer a kernel would see whose row r continued into row r + 1: L more cells per row, the next row's first"""
    H, W = columns.shape
    out = np.zeros((H, W + L), dtype=U64)
    out[:, :W] = columns
    out[:-1, W:] = columns[1:, :L]
    return out


# ---- the gate -------------------------------------------------------------------------------------------------------------------------
def gate_layer(centre, neighbour):
    """5 x 5 cells: the 3 x 3 block in the middle at ground `centre`, but the cell right of the middle one at `neighbour`"""
    g = np.full((5, 5), 255, dtype=np.int64)
    g[1:4, 1:4] = centre
    g[2, 3] = neighbour
    return from_grounds(g)


# (name, centre, neighbour, K, min_cells): the middle cell (2, 2), L = 1, rise = 0.  `in`: the neighbour lies at |g_n - g| = K; `out`: at K + 1.
GATES = [("gate6_in_above", 20, 26, 6, 3), ("gate6_out_above", 20, 27, 6, 3), ("gate6_in_below", 20, 14, 6, 3), ("gate6_out_below", 20, 13, 6, 3),
         ("gate0_in", 20, 20, 0, 9), ("gate0_out", 20, 21, 0, 9),  # K = 0 admits only level cells: what depends on the neighbour is the fit (n = 9 = min_cells)
         ("gate63_in", 0, 63, 63, 3), ("gate62_out", 0, 63, 62, 3), ("gate63_in_below", 63, 0, 63, 3)]


# ---- min_cells ------------------------------------------------------------------------------------------------------------------------
def min_cells_layer():
    """9 x 9 cells, seven of them known in the window (L = 2) of the middle cell (4, 4), not on one line, on a tilt; and a diagonal of
    five cells apart from them, around (4, 4) of the second layer: n = 5 and D = 0"""
    g = np.full((9, 9), 255, dtype=np.int64)
    for x, y in ((4, 4), (2, 2), (6, 2), (3, 5), (5, 6), (6, 4), (2, 6)):
        g[y, x] = 10 + x
    d = np.full((9, 9), 255, dtype=np.int64)
    for k in range(2, 7):
        d[k, k] = 10 + k
    return from_grounds(g), from_grounds(d)


# ---- the comparison -------------------------------------------------------------------------------------------------------------------
def ramp_layer():
    """20 x 20 cells, all known, the ground equal to x: a = 1 and b = 0 exactly, in every window"""
    return from_grounds(np.tile(np.arange(20), (20, 1)))


def level_layer():
    return from_grounds(np.full((20, 20), 7))


RAMP_LIMITS = [(1, 1), (1023, 1024), (65535, 65535), (65534, 65535), (0, 1), (0, 65535)]  # rise, run: SLOPE exactly where rise / run < 1


# ---- the widths -----------------------------------------------------------------------------------------------------------------------
WIDE_SPLIT = 12


def wide_layer():
    """25 x 25 cells, all known: ground 0 up to x = 12 and 63 beyond - for cell (12, y), 8 <= y <= 16, a full window of L = 8 split at
    dx > 0"""
    g = np.zeros((25, 25), dtype=np.int64)
    g[:, WIDE_SPLIT + 1:] = 63
    return from_grounds(g)


WIDE_LIMITS = [(65535, 65535), (65534, 65535), (65535, 65534), (65535, 1), (1, 65535)]

# ---- random columns, and the drive ----------------------------------------------------------------------------------------------------
# ((S, H), slope): the least of everything; the prototype's; the widest window with every ground admitted and any tilt marked; a full
# window demanded; no gate
RANDOM_CONFIGS = [((2, 8), (1, 3, 3, 1, 2)), ((2, 8), (4, 6, 12, 596, 1024)), ((0, 64), (8, 63, 3, 0, 1)), ((62, 63), (8, 63, 289, 65535, 1)), ((5, 64), (2, 0, 5, 3, 7))]
DRIVE_PARAMS, DRIVE_SLOPE = (2, 24), (4, 12, 12, 596, 1024)  # 596 / 1024 slabs per cell: 20 degrees on the drive's 0.1 m cells and 0.0625 m slabs


@functools.lru_cache(maxsize=None)
def drive_columns():
    """(cfg, frames, the columns after the drive) of tests/elev_cases.py's random_drive, by the restatement"""
    cfg, frames = ec.random_drive()
    after, _ = ec.reference_run(cfg, frames)
    return cfg, frames, after[-1]


def small_cases():
    """every hand-made case: (name, columns, (S, H), slope, rectangles)"""
    cases = [(name, columns, NO_STEP, (4, 63, 3, 0, 1), [None]) for name, columns in collinear_layers()]
    for side in SQUARE_SIDES:
        for slope in SQUARE_SLOPES:
            rects = [None] + ([(side - 9, 3, 9, side - 3), (15, 15, 2, 2)] if side > 16 else [(side - 1, side - 1, 1, 1)])
            cases.append(("square%d_L%d" % (side, slope[0]), tilted_square(side, 100 + side), (2, 8), slope, rects))
    columns, slope = wrap_layer()
    cases.append(("wrap", columns, NO_STEP, slope, [None, (WRAP_CELL[0], WRAP_CELL[1], 1, 1), (17, 0, 3, 12)]))
    for name, centre, neighbour, K, min_cells in GATES:
        cases.append((name, gate_layer(centre, neighbour), NO_STEP, (1, K, min_cells, 0, 1), [None]))
    tilt, diagonal = min_cells_layer()
    cases += [("min_cells_met", tilt, NO_STEP, (2, 63, 7, 0, 1), [None]), ("min_cells_missed", tilt, NO_STEP, (2, 63, 8, 0, 1), [None]),
              ("on_one_line", diagonal, NO_STEP, (2, 63, 3, 0, 1), [None])]
    for rise, run in RAMP_LIMITS:
        cases.append(("ramp_%d_%d" % (rise, run), ramp_layer(), NO_STEP, (2, 63, 3, rise, run), [None, (17, 2, 3, 5)]))
    cases.append(("level_rise0", level_layer(), NO_STEP, (2, 63, 3, 0, 1), [None]))
    for rise, run in WIDE_LIMITS:
        cases.append(("wide_%d_%d" % (rise, run), wide_layer(), NO_STEP, (8, 63, 289, rise, run), [None, (WIDE_SPLIT, 8, 1, 9)]))
    return cases


def random_cases():
    return [("random_%s_%d" % (kind, k), ec.random_columns(kind), params, slope, ec.RECTS) for kind in ("dense", "sparse", "zero")
            for k, (params, slope) in enumerate(RANDOM_CONFIGS)]


def all_cases():
    return small_cases() + random_cases()


RADIUS_RECTS = [None, (15, 15, 2, 2)]


def radius_cases():
    """One case per radius the fit kernels are instantiated for, L = 1 .. 8 - the suites above only ever launch 1, 2, 4 and 8 - on one
    33 x 33 layer: three tiles per side, the last overhanging, and at L = 8 a halo wider than one trip of the tile's staging loop.  Every
    ground admitted, the fewest cells, the squares' limit."""
    columns = tilted_square(33, 133)
    return [("radius_L%d" % L, columns, (2, 8), (L, 63, 3, 4, 5), RADIUS_RECTS) for L in range(1, 9)]


_expected = {}


def expected(case):
    """the restatement's result for a case's full layer - computed once per case and shared; nobody changes it"""
    name, columns, (S, H), slope, _ = case
    if name not in _expected:
        _expected[name] = sr.classify(columns, S, H, slope)
    return _expected[name]


def check_result(case, rect, got, got_ground=None, got_fit=None, got_counts=None):
    """a result of one rectangle of a case against the restatement: np.array_equal and == throughout"""
    name, columns, _, _, _ = case
    want = expected(case)
    r = rect or (0, 0, columns.shape[1], columns.shape[0])
    assert got.dtype == np.int8 and got.shape == (r[3], r[2]), (name, rect)
    assert np.array_equal(got, er.restrict(want.classes, r)), (name, rect)
    if got_ground is not None:
        assert got_ground.dtype == np.uint8 and np.array_equal(got_ground, er.restrict(want.ground, r)), (name, rect)
    if got_fit is not None:
        assert got_fit.dtype == np.int64 and np.array_equal(got_fit, er.restrict(want.fit, r)), (name, rect)
    if got_counts is not None:
        assert got_counts == sr.counts(want, r), (name, rect, got_counts, sr.counts(want, r))
