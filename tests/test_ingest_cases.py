"""The premises of tests/ingest_cases.py, proved on the CPU, so that the GPU tests of tests/test_gpu_ingest_regimes.py compare
against something that is known to be right and known to bite: the oracle's ingest equals an independent numpy decode bit for
bit on every case, the stamps' extrema sit at the records the case names, the condition on stamps holds, the table's `aligned`
and `wide` columns follow from the layouts, every placement and stamp set is in the table, and no point of a pre-step case has a
range so close to a crop bound that a rounding difference could flip the survivor count."""
import numpy as np
import pytest

import ingest_cases as ic
from checkers import okicp


@pytest.mark.parametrize("case", ic.DECODE_CASES, ids=repr)
def test_oracle_equals_numpy_decode_and_the_extrema_sit_where_the_case_says(case):
    m = case.build()
    L = case.layout
    xyz, st, mm = okicp.ingest(*m.args)
    exp_xyz, exp_st, exp_mm = ic.numpy_decode(m.rec, L.stamp)
    finite = ic.assert_same_cloud(xyz, exp_xyz)  # (as bit patterns: signed zeros count)
    assert finite.all() != case.invalid
    if L.stamp is None:
        assert st is None and mm == (0.0, 0.0) and m.imin is None
        return
    np.testing.assert_array_equal(st, exp_st)
    assert mm == exp_mm
    # the condition on stamps, on the values the record holds
    t = m.rec["t"].astype(np.float64)
    assert np.all(np.isfinite(t)) and t.min() > -0.5 and t.max() < 1.8e19
    sec = ic.stamp_seconds(t)
    if case.stamps in ic.CONSTANT_SETS:
        assert mm[0] == mm[1] and np.all(np.isnan(st)) and m.imin is None
        return
    assert (m.imin, m.imax) == case.extrema_at() and m.imin != m.imax
    assert sec[m.imin] == mm[0] and sec[m.imax] == mm[1] and mm[0] < mm[1]
    assert np.flatnonzero(sec == mm[0]).tolist() == [m.imin] and np.flatnonzero(sec == mm[1]).tolist() == [m.imax]
    assert st[m.imin] == 0.0 and st[m.imax] == 1.0
    assert not np.all(np.diff(sec) >= 0)  # placed by a permutation, not sorted
    if case.stamps in ("velodyne", "mixed_sign"):
        assert mm[0] < 0.0  # ordered_key's branch for negative doubles
    if case.stamps in ("boundary", "epoch_mix", "ns_f32"):
        converts = np.floor(t + 0.5) >= 1e10
        assert converts.any() and not converts.all()  # a cloud that mixes converting and non-converting stamps
    if case.stamps == "boundary":
        assert mm == (0.25, float(np.nextafter(9_999_999_999.5, 0.0))) and 9_999_999_999.5 * 1e-9 in sec and 10.0 in sec and 9_999_999_999.4 in sec
    if case.stamps == "u32_full":
        assert mm == (0.0, 4294967295.0)  # never nanoseconds


def test_the_tables_columns_follow_from_the_layouts():
    """`aligned` as kicp.h words it - every field at a multiple of its size, point_step a multiple of every field's size -, `wide`,
    the minimum launch count; the one-term neighbours of the predicate are what their names say; the limits of the LDS path and the
    clamp of piece_records are in the table; every short layout has a variant whose last field ends at point_step."""
    for L in ic.LAYOUTS:
        fields = [(L.x, 4), (L.y, 4), (L.z, 4)] + ([(L.t, 8 if L.stamp == ic.F64 else 4)] if L.stamp else [])
        assert L.aligned == int(all(o % s == 0 and L.step % s == 0 for o, s in fields)), L.name
        assert L.wide == int(L.step > 128)
        assert all(o + s <= L.step for o, s in fields)
    terms = {  # which terms of the predicate fail: (point_step % 4, offsets % 4, stamp offset % size, point_step % stamp size)
        "s20_f64_at_12": (0, 0, 1, 1), "s24_f64_at_16": (0, 0, 0, 0), "s28_f64_at_16": (0, 0, 0, 1), "s18_none": (1, 0, 0, 0),
        "s16_x_at_2": (0, 1, 0, 0), "packed16_u32": (0, 0, 0, 0), "packed16_f32": (0, 0, 0, 0), "packed16_none": (0, 0, 0, 0)}
    for name, want in terms.items():
        L = ic.LAYOUT[name]
        sb = 8 if L.stamp == ic.F64 else 4
        got = (int(L.step % 4 != 0), int(any(o % 4 for o in (L.x, L.y, L.z))), int(bool(L.stamp) and L.t % sb != 0), int(bool(L.stamp) and L.step % sb != 0))
        assert got == want and L.aligned == int(not any(want)), name
    steps = {L.step for L in ic.LAYOUTS}
    assert {127, 128, 129, 132, 144, 256, 2052} <= steps
    assert ic.piece_records(2052) == 256 and ic.piece_records(16) == 32768
    assert {(L.step, L.aligned) for L in ic.LAYOUTS} >= {(127, 0), (128, 0), (128, 1), (129, 0), (132, 1), (144, 1), (256, 1), (2052, 1)}
    for L in ic.LAYOUTS:
        if L.wide:
            assert L.stamp and L.t + (8 if L.stamp == ic.F64 else 4) == L.step, L.name  # the stamp ends exactly at point_step
    short_keys = {(L.step, L.stamp) for L in ic.LAYOUTS if not L.wide}
    assert short_keys == {(L.step, L.stamp) for L in ic.LAYOUTS if not L.wide and L.ends_at_step}
    by = {}
    for c in ic.DECODE_CASES:
        by.setdefault(c.layout.name, set()).add(c.n)
        assert c.min_launches == -(-c.n // c.piece_records)
    for L in ic.LAYOUTS:
        pr = ic.piece_records(L.step)
        assert {255, 256, 512, pr - 1, pr, pr + 1, 2 * pr + 1} <= by[L.name], L.name
    launches = {c.n: c.min_launches for c in ic.DECODE_CASES if c.layout.step == 2052}
    assert launches[1000] == 4 and launches[3000] == 12


def test_every_stamp_set_meets_every_placement():
    seen = {(c.stamps, c.placement) for c in ic.DECODE_CASES if isinstance(c.placement, str)}
    for stamps in ic.STAMP_SETS:
        if stamps in ic.CONSTANT_SETS:
            assert any(c.stamps == stamps for c in ic.DECODE_CASES)
            continue
        for placement in ic.PLACEMENTS:
            assert (stamps, placement) in seen, (stamps, placement)
    # both float widths of the negative sets
    assert {c.layout.stamp for c in ic.DECODE_CASES if c.stamps == "velodyne"} == {ic.F32, ic.F64}
    # the look-ahead cases' extrema sit in tiles of piece 0 beyond the 48 workgroups a look-ahead launch has by default
    for c in ic.AHEAD_CASES[2:]:
        for i in c.extrema_at():
            assert i < c.piece_records and i // 256 >= 48
    assert sorted(i // 256 // 48 for c in ic.AHEAD_CASES[2:] for i in c.extrema_at()) == [1, 1, 2, 2]  # second and third round


@pytest.mark.parametrize("run", ic.prestep_runs(), ids=lambda r: "%s-deskew%d-min%g" % (r[0].name, r[1], r[2]))
def test_no_range_of_a_prestep_case_sits_on_a_crop_bound(run):
    """Ranges as the oracle computes them (deskewed where the run deskews): none within 1e-9 of max_range or min_range, so a
    last-bit difference in the deskewed point cannot flip a survivor count (nor, a voxel edge being as far, a downsample count).  One exception, which is exact and not a rounding
    matter: without deskewing a (0, 0, 0) record has range 0.0 == min_range 0.0 on either side and is dropped (`>` is strict)."""
    case, deskew, min_range = run
    rel, ext = ic.prestep_poses()
    m = case.build()
    xyz, st, _ = okicp.ingest(*m.args)
    finite = np.all(np.isfinite(xyz), axis=1)
    zero = np.all(xyz == 0.0, axis=1)
    assert case.invalid == bool((~finite).any()) and case.invalid == bool(zero.any())
    if case.invalid:
        assert (~finite).sum() == 3 * (case.n // 20) and zero.sum() == case.n // 20 and finite[[m.imin, m.imax]].all() and not zero[[m.imin, m.imax]].any()
    moved = okicp.preprocess(xyz, st, rel, np.inf, -1.0, deskew)  # every point with a finite range, in input order
    assert len(moved) == finite.sum()
    r = np.linalg.norm(moved, axis=1)
    exact = zero[finite] & (not deskew)
    assert np.all(r[exact] == 0.0)
    for bound in (ic.MAX_RANGE, min_range):
        assert np.all(np.abs(r[~exact] - bound) > 1e-9)
    kept = okicp.preprocess(xyz, st, rel, ic.MAX_RANGE, min_range, deskew)
    assert 0 < len(kept) < finite.sum()
    # ... nor does a survivor's coordinate in the base frame sit on a voxel edge of either downsample (the counts of the chained Frame)
    base = okicp.se3_act(ext, kept)
    for voxel in (ic.VOXEL_A, ic.VOXEL_B):
        assert np.abs(base / voxel - np.round(base / voxel)).min() * voxel > 1e-9
    if case.invalid and deskew and min_range == 0.0:
        # deskewing moves a (0, 0, 0) record off the origin: the reference keeps it
        assert np.sum((r > min_range) & (r < ic.MAX_RANGE) & zero[finite]) >= 1
