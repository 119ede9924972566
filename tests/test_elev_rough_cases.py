"""What the cases of the class ROUGH (tests/elev_rough_cases.py) are there for, proved on the CPU with the restatement
(tests/elev_rough_ref.py): each case enters its regime, and the restatement's answer changes without the thing the case is for - so a
kernel or host code that gets that thing wrong cannot agree with it.  No GPU, no library."""
import numpy as np
import pytest

import clearance_ref as cr
import elev_ref as er
import elev_rough_cases as rc
import elev_rough_ref as rr
import elev_slope_cases as sc
import elev_slope_ref as sr

CASES = {case[0]: case for case in rc.small_cases()}


def test_an_exact_plane_has_no_residual():
    for L in (1, 2, 8):
        want = rc.expected(CASES["plane_L%d" % L])
        assert want.has_fit.all() and all(int(q) == 0 for q in want.Q.ravel()) and not want.rough.any() and (want.classes == 0).all()
        assert CASES["plane_L%d" % L][4] == (0, 1)  # even at num = 0
        assert all(int(a) == int(d) and int(b) == 2 * int(d) for d, a, b in zip(want.D.ravel(), want.Da.ravel(), want.Db.ravel()))  # a = 1, b = 2
        assert not np.array_equal(want.fit[:, :, 3], want.fit[:, :, 0]) and (want.fit[:, :, 4] == want.sums["n"]).all()


def test_one_raised_cell_by_hand_and_the_comparison_is_strict():
    x, y = rc.BUMP_CELL
    want = rc.expected(CASES["bump_L1"])
    assert tuple(int(v) for v in want.fit[y, x]) == rc.BUMP_FIT and int(want.Dc[y, x]) == -864 and int(want.szz[y, x]) == 102
    assert want.rough[y - 1:y + 2, x - 1:x + 2].all() and want.rough.sum() == 9  # the cell and its eight neighbours see it
    d, _, _, q, n = rc.BUMP_FIT
    num, den = rc.BUMP_EQUAL
    assert q * den == num * n * d
    equal, below = rc.expected(CASES["bump_equal"]), rc.expected(CASES["bump_below"])
    assert not equal.rough[y, x] and equal.classes[y, x] == 0 and int(equal.left[y, x]) == int(equal.right[y, x])
    assert CASES["bump_below"][4] == (num - 1, den) and below.rough[y, x] and below.classes[y, x] == 100 and below.rough.sum() == 1


def test_the_checkerboard_needs_a_128_bit_left_side():
    x, y = rc.WIDE_CELL
    want = rc.expected(CASES["checkerboard"])
    num, den = CASES["checkerboard"][4]
    q, d, n = int(want.Q[y, x]), int(want.D[y, x]), int(want.sums["n"][y, x])
    assert n == 289 and want.has_fit[y, x] and q >= 1 << 51 and q < 1 << 55 and q <= d * int(want.szz[y, x])
    left, right = q * den, num * n * d
    assert left == int(want.left[y, x]) and right == int(want.right[y, x])
    assert left >= 1 << 64 and right < 1 << 59 and left > right and left % (1 << 64) <= right  # wrapped to 64 bits it falls below the right side
    assert want.rough[y, x] and want.classes[y, x] == 100 and not want.step[y, x] and not want.slope.any()
    never = rc.expected(CASES["checkerboard_never"])  # 65 535 slabs^2: above any residual
    assert not never.rough.any() and int(never.left[y, x]) < int(never.right[y, x])
    split = rc.expected(CASES["split"])  # the slope suite's wide layer: the determinants at their widths
    sx = sc.WIDE_SPLIT
    assert abs(int(split.Da[12, sx])) > 1 << 32 and abs(int(split.Dc[12, sx])) > 1 << 32 and abs(int(split.Da[12, sx]) * int(split.sums["sxz"][12, sx])) > 1 << 48
    assert split.rough[12, sx] and int(split.Q[12, sx]) > 1 << 48
    # exact arithmetic: 0 <= Q <= D Szz < 2^55 on every fitted cell of every case
    for case in rc.all_cases():
        w = rc.expected(case)
        assert all(0 <= int(q) <= int(d) * int(s) < 1 << 55 for q, d, s in zip(w.Q[w.has_fit].ravel(), w.D[w.has_fit].ravel(), w.szz[w.has_fit].ravel())), case[0]


def test_three_cells_lines_and_min_cells():
    three = rc.expected(CASES["three_cells"])
    assert three.has_fit[2, 2] and three.has_fit.sum() == 1 and int(three.sums["n"][2, 2]) == 3 and int(three.Q[2, 2]) == 0 and not three.rough.any()  # (the other two see two cells)
    assert all(int(s) > 0 for s in three.szz[three.has_fit])  # grounds far apart: Szz is large, the plane takes all of it
    met, missed, line = (rc.expected(CASES[name]) for name in ("min_cells_met", "min_cells_missed", "on_one_line"))
    mid = (4, 4)
    assert met.has_fit[mid] and int(met.sums["n"][mid]) == 7 and met.fit[mid][4] == 7
    assert not missed.has_fit[mid] and int(missed.D[mid]) > 0 and not missed.fit.any() and not missed.rough.any()
    assert int(line.sums["n"][mid]) == 5 and int(line.D[mid]) == 0 and not line.fit.any() and not line.rough.any() and int(line.szz[mid]) > 0
    for name in ("one_cell", "one_row", "one_column"):
        want = rc.expected(CASES[name])
        assert not want.has_fit.any() and not want.fit.any() and not want.rough.any() and (want.classes == 0).all()


def test_the_gate_keeps_an_outlier_out_of_szz():
    name, columns, (S, H), slope, rough, _ = CASES["gate_out"]
    want = rc.expected(CASES["gate_out"])
    mid = rc.GATE_MID
    assert int(want.sums["n"][mid]) == 8 and want.has_fit[mid] and int(want.Q[mid]) == 0 and not want.rough[mid] and want.classes[mid] == 0
    # the ninth cell let into Szz alone: the answer flips
    leaky = rr.szz(want.ground, slope[0], slope[1], admit_beyond_gate=True)
    assert int(leaky[mid]) == 49 and int(want.szz[mid]) == 0
    q, _ = rr.residual(want.sums, leaky, want.D, want.Da, want.Db)
    assert int(q[mid]) == 49 * int(want.D[mid]) > 0  # Q den > num n D at num = 0: ROUGH
    inside = rc.expected(CASES["gate_in"])  # at |g_n - g| = K it counts
    assert int(inside.sums["n"][mid]) == 9 and inside.rough[mid] and int(inside.szz[mid]) == 36


@pytest.mark.parametrize("side", sc.SQUARE_SIDES)
@pytest.mark.parametrize("slope", sc.SQUARE_SLOPES, ids=["L1", "L8"])
def test_tilted_squares_are_rough_on_both_sides_of_every_tile_border(side, slope):
    want = rc.expected(CASES["square%d_L%d" % (side, slope[0])])
    only = want.rough & ~want.body & ~want.step & ~want.slope
    assert only.any() and (want.has_fit & ~want.rough).any() and (want.ground == 255).any()
    for border in (16, 32):
        if side > border:
            assert want.has_fit[:, border - 1].any() and want.has_fit[:, border].any() and want.has_fit[border - 1, :].any() and want.has_fit[border, :].any()
    assert np.array_equal(want.fit[:, :, :3], sc.expected([c for c in sc.small_cases() if c[0] == CASES["square%d_L%d" % (side, slope[0])][0]][0]).fit)


def test_a_cell_decides_rough_across_every_tile_border():
    name, columns, (S, H), slope, rough, _ = CASES["borders"]
    want = rc.expected(CASES["borders"])
    assert want.has_fit.all() and not want.slope.any() and not want.step.any()
    for bump, witness in rc.BORDER_PAIRS:
        (bx, by), (wx, wy) = bump, witness
        assert max(abs(bx - wx), abs(by - wy)) == 1 and (bx // 16 != wx // 16 or by // 16 != wy // 16)  # neighbours that a tile border parts
        assert want.rough[wy, wx] and want.classes[wy, wx] == 100
        without = rr.classify(rc.border_layer(without=bump), S, H, slope, rough)
        assert not without.rough[wy, wx] and without.classes[wy, wx] == 0
    crossed = {(min(b[0], w[0]) // 16 * 16 + 16 if b[0] // 16 != w[0] // 16 else 0, min(b[1], w[1]) // 16 * 16 + 16 if b[1] // 16 != w[1] // 16 else 0)
               for b, w in rc.BORDER_PAIRS}
    assert {(16, 0), (32, 0), (0, 16), (0, 32), (16, 16), (32, 32)} <= crossed


def test_the_halo_must_not_run_past_a_rows_end():
    name, columns, (S, H), slope, rough, _ = CASES["wrap"]
    x, y = sc.WRAP_CELL
    want = rc.expected(CASES["wrap"])
    assert x == sc.WRAP_W - 1 and want.has_fit[y, x] and int(want.Q[y, x]) == 0 and not want.rough[y, x] and want.classes[y, x] == 0
    wrapped = rr.classify(sc.wrapped_view(columns, slope[0]), S, H, slope, rough)
    assert wrapped.rough[y, x] and wrapped.classes[y, x] == 100 and not wrapped.slope[y, x]


def test_random_columns_enter_every_class_and_one_case_all_six():
    seen, all_six = np.zeros(6, dtype=np.int64), []
    for case in rc.random_cases():
        want = rc.expected(case)
        words = rr.counts(want)
        seen += np.array(words)
        if all(w > 0 for w in words):
            all_six.append(case[0])
        if "zero" in case[0]:
            assert (want.classes == -1).all() and not want.fit.any()
        # not ROUGH only => the slope limit's value; the fit's first three are the slope limit's
        only = want.rough & ~want.body & ~want.step & ~want.slope
        slope_only = sr.classify(case[1], *case[2], case[3])
        assert np.array_equal(want.classes[~only], slope_only.classes[~only]) and (want.classes[only] == 100).all() and (slope_only.classes[only] == 0).all()
        assert np.array_equal(want.fit[:, :, :3], slope_only.fit)
    assert (seen > 0).all() and "random_sparse_1" in all_six


def test_the_drive_not_rough_only_means_unchanged_and_a_frame_stays_in_its_window():
    cfg, frames, columns = sc.drive_columns()
    (S, H), slope, rough = sc.DRIVE_PARAMS, sc.DRIVE_SLOPE, rc.DRIVE_ROUGH
    assert rough == rr.rough_limit(cfg["slab"], cfg["slab"] * np.sqrt(0.5))
    want = rr.classify(columns, S, H, slope, rough)
    only = want.rough & ~want.body & ~want.step & ~want.slope
    print("drive:", rr.counts(want))
    assert only.sum() > 50 and (want.has_fit & ~want.rough).sum() > 100 and all(w > 0 for w in rr.counts(want))
    assert np.array_equal(want.classes[~only], want.classes_slope[~only]) and (want.classes[only] == 100).all() and (want.classes_slope[only] == 0).all()
    more = columns.copy()
    pts, pose, sensor = frames[0]
    er.integrate(cfg, more, pts + np.array([0.0, 0.0, 0.4]), pose, sensor)
    after = rr.classify(more, S, H, slope, rough)
    x0, y0, w, h = cr.grown(er.window(cfg, pose, sensor), max(1, slope[0]), cfg["width"], cfg["height"])
    outside = np.ones(columns.shape, dtype=bool)
    outside[y0:y0 + h, x0:x0 + w] = False
    assert outside.any() and np.array_equal(after.classes[outside], want.classes[outside]) and np.array_equal(after.fit[outside], want.fit[outside])
    assert not np.array_equal(after.classes, want.classes) and not np.array_equal(after.fit, want.fit)
