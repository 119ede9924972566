"""What the slope limit's cases (tests/elev_slope_cases.py) are there for, proved on the CPU with the restatement
(tests/elev_slope_ref.py): each case enters its regime, and the restatement's answer changes without the thing the case is for - so a
kernel or host code that gets that thing wrong cannot agree with it.  No GPU, no library."""
import numpy as np
import pytest

import clearance_ref as cr
import elev_cases as ec
import elev_ref as er
import elev_slope_cases as sc
import elev_slope_ref as sr

CASES = {case[0]: case for case in sc.small_cases()}


def test_a_line_of_cells_has_no_fit():
    for name in ("one_cell", "one_row", "one_column"):
        want = sc.expected(CASES[name])
        assert (want.ground != 255).all() and (want.sums["n"] >= (1 if name == "one_cell" else 5)).all()
        assert all(int(d) == 0 for d in want.D.ravel()) and not want.has_fit.any() and not want.slope.any() and not want.fit.any()
    assert any(int(v) != 0 for v in sc.expected(CASES["one_row"]).sums["sxz"].ravel())  # the grounds do rise along the line


@pytest.mark.parametrize("side", sc.SQUARE_SIDES)
@pytest.mark.parametrize("slope", sc.SQUARE_SLOPES, ids=["L1", "L8"])
def test_tilted_squares_straddle_every_tile_border(side, slope):
    want = sc.expected(CASES["square%d_L%d" % (side, slope[0])])
    fitted = want.has_fit
    assert (fitted & want.slope).any() and (fitted & ~want.slope).any() and (want.ground == 255).any() and want.step.any()
    for border in (16, 32):
        if side > border:  # cells with a fit on both sides of the border, in both directions
            assert fitted[:, border - 1].any() and fitted[:, border].any() and fitted[border - 1, :].any() and fitted[border, :].any()
    # the fit of a border cell reaches across: without the cells beyond the border the answer is another
    if side > 16:
        name, columns, (S, H), cfg, _ = CASES["square%d_L%d" % (side, slope[0])]
        cut = sr.classify(columns[:16, :16], S, H, cfg)
        assert not np.array_equal(cut.fit, want.fit[:16, :16])
        assert np.array_equal(cut.fit[:16 - slope[0], :16 - slope[0]], want.fit[:16 - slope[0], :16 - slope[0]])


def test_the_halo_must_not_run_past_a_rows_end():
    name, columns, (S, H), slope, _ = CASES["wrap"]
    x, y = sc.WRAP_CELL
    want = sc.expected(CASES["wrap"])
    assert x == sc.WRAP_W - 1 and want.has_fit[y, x] and not want.slope[y, x] and want.classes[y, x] == 0 and int(want.sums["n"][y, x]) == 28
    wrapped = sr.classify(sc.wrapped_view(columns, slope[0]), S, H, slope)
    assert wrapped.slope[y, x] and wrapped.classes[y, x] == 100 and int(wrapped.sums["n"][y, x]) == 28 + 21


def test_the_gate_admits_k_and_refuses_k_plus_one():
    mid = (2, 2)
    for name in ("gate6_in_above", "gate6_in_below", "gate63_in", "gate63_in_below"):
        want = sc.expected(CASES[name])
        assert int(want.sums["n"][mid]) == 9 and want.slope[mid] and want.classes[mid] == 100 and not want.body.any(), name
        # SLOPE only - but where the middle cell lies 63 slabs over its neighbour: the higher cell of that edge is STEP at every S
        assert want.step[mid] == (name == "gate63_in_below"), name
    for name in ("gate6_out_above", "gate6_out_below", "gate62_out"):
        want = sc.expected(CASES[name])
        assert int(want.sums["n"][mid]) == 8 and want.has_fit[mid] and not want.slope[mid] and want.classes[mid] == 0, name
    inside, outside = sc.expected(CASES["gate0_in"]), sc.expected(CASES["gate0_out"])
    assert int(inside.sums["n"][mid]) == 9 and inside.has_fit[mid] and inside.fit[mid][0] > 0 and not inside.slope.any()
    assert int(outside.sums["n"][mid]) == 8 and not outside.has_fit[mid] and not outside.fit[mid].any()
    assert {case[3][1] for case in CASES.values() if case[0].startswith("gate")} == {0, 6, 62, 63}


def test_min_cells_is_met_exactly_or_missed_by_one():
    mid = (4, 4)
    met, missed, line = (sc.expected(CASES[name]) for name in ("min_cells_met", "min_cells_missed", "on_one_line"))
    assert int(met.sums["n"][mid]) == 7 == CASES["min_cells_met"][3][2] and met.has_fit[mid] and met.slope[mid] and met.classes[mid] == 100
    assert CASES["min_cells_missed"][3][2] == 8 and not missed.has_fit[mid] and not missed.slope.any() and missed.classes[mid] == 0 and int(missed.D[mid]) > 0
    assert int(line.sums["n"][mid]) == 5 >= CASES["on_one_line"][3][2] and int(line.D[mid]) == 0 and not line.has_fit.any() and not line.slope.any()
    assert int(line.Da[mid]) == 0 and int(line.sums["sxz"][mid]) != 0  # a tilt along the line, and nothing to divide by


def test_the_comparison_is_strict_and_exact():
    for rise, run in sc.RAMP_LIMITS:
        want = sc.expected(CASES["ramp_%d_%d" % (rise, run)])
        assert want.has_fit.all() and all(int(a) == int(d) and int(b) == 0 for d, a, b in zip(want.D.ravel(), want.Da.ravel(), want.Db.ravel()))  # a = 1, b = 0
        assert want.slope.all() if rise < run else not want.slope.any(), (rise, run)
        assert not want.body.any() and not want.step.any()
    level = sc.expected(CASES["level_rise0"])
    assert level.has_fit.all() and not level.slope.any() and (level.classes == 0).all()  # rise = 0 marks no level patch
    assert {(1, 1), (1023, 1024), (0, 1)} <= set(sc.RAMP_LIMITS)


def test_the_wide_case_needs_every_bit_of_the_integers():
    x, flipped = sc.WIDE_SPLIT, 0
    for rise, run in sc.WIDE_LIMITS:
        want = sc.expected(CASES["wide_%d_%d" % (rise, run)])
        for y in range(8, 17):
            assert int(want.sums["n"][y, x]) == 289 and want.has_fit[y, x]
            left, right = int(want.left[y, x]), int(want.right[y, x])
            assert int(want.D[y, x]) > 1 << 32 and abs(int(want.Da[y, x])) > 1 << 32 and int(want.D[y, x]) < 1 << 34 and abs(int(want.Da[y, x])) < 1 << 41
            assert max(left, right) >= 1 << 64 and left < 1 << 115 and right < 1 << 100
            flipped += ((left & (2 ** 64 - 1)) > (right & (2 ** 64 - 1))) != (left > right)
        assert want.slope[8:17, x].all() == (want.left[12, x] > want.right[12, x])
    assert flipped >= 1  # comparing the low 64 bits gives the other verdict
    verdicts = {limit: bool(sc.expected(CASES["wide_%d_%d" % limit]).slope[12, x]) for limit in sc.WIDE_LIMITS}
    assert verdicts[(65535, 1)] is False and verdicts[(1, 65535)] is True


def test_random_columns_enter_every_class():
    seen = np.zeros(5, dtype=np.int64)
    for case in sc.random_cases():
        want = sc.expected(case)
        seen += np.array(sr.counts(want))
        if "zero" in case[0]:
            assert (want.classes == -1).all() and not want.fit.any()
    assert (seen > 0).all()
    full = sc.expected([c for c in sc.random_cases() if c[0] == "random_dense_3"][0])
    assert full.has_fit.any() and (full.sums["n"][full.has_fit] == 289).all()  # min_cells = 289: only full windows fit


def test_the_drive_not_slope_only_means_unchanged_and_a_frame_stays_in_its_window():
    cfg, frames, columns = sc.drive_columns()
    (S, H), slope = sc.DRIVE_PARAMS, sc.DRIVE_SLOPE
    assert slope[3:] == sr.slope_limit(cfg["cell"], cfg["slab"], np.tan(np.deg2rad(20.0)))
    want = sr.classify(columns, S, H, slope)
    plain = er.classify(columns, S, H)[0]
    only = want.slope & ~want.body & ~want.step
    assert only.sum() > 50 and (want.has_fit & ~want.slope).sum() > 1000
    assert np.array_equal(want.classes[~only], plain[~only]) and (want.classes[only] == 100).all() and (plain[only] == 0).all()
    more = columns.copy()
    pts, pose, sensor = frames[0]
    er.integrate(cfg, more, pts + np.array([0.0, 0.0, 0.4]), pose, sensor)
    after = sr.classify(more, S, H, slope)
    x0, y0, w, h = cr.grown(er.window(cfg, pose, sensor), max(1, slope[0]), cfg["width"], cfg["height"])
    outside = np.ones(columns.shape, dtype=bool)
    outside[y0:y0 + h, x0:x0 + w] = False
    assert outside.any() and np.array_equal(after.classes[outside], want.classes[outside]) and np.array_equal(after.fit[outside], want.fit[outside])
    assert not np.array_equal(after.classes, want.classes) and not np.array_equal(after.fit, want.fit)
