"""The case table of the PointCloud2 ingest's regime tests, shared by tests/test_ingest_cases.py (CPU: the premises of every case)
and tests/test_gpu_ingest_regimes.py (GPU: k_ingest / ingest_run and the consumers of what they decode).

A case is a record layout, a stamp set, a size and the records at which the stamps' minimum and maximum sit.  Layouts: records
around the 128-byte limit of the LDS path (127, 128, 129) and far beyond it (132, 144, 256, 2052 - the last one so long that a piece
is one workgroup), and the one-term neighbours of the `aligned` predicate; in most of them the last field ends exactly at
point_step.  Stamp sets: negative (Velodyne-like) and mixed-sign stamps, the nanosecond rule's boundary values, clouds that mix
converting and non-converting stamps, full-range UINT32, constant stamps.  Every set is placed by a fixed permutation - never sorted -
and its two extrema are then swapped to the records the case names: a tile edge, a piece edge, a one-record tail piece, a tile that a
look-ahead launch visits on a later round of its tile loop.  Padding and foreign fields hold junk bytes, x y z are float32 in +-80.

Condition on stamps, asserted by the builder: every stamp is finite, > -0.5 and < 1.8e19.  Outside that range the reference's
static_cast<uint64_t>(round(stamp)) (TimeStampHandler.cpp:60) is undefined, so there is nothing to compare against; NaN and infinite
stamps are out of scope for the same reason.

PIECE_BYTES restates the rule include/kicp.h documents for "ingest_piece_records"; the GPU tests assert it against that counter."""
import zlib

import numpy as np

U32, F32, F64 = 6, 7, 8  # sensor_msgs::msg::PointField datatype codes
_FMT = {U32: "<u4", F32: "<f4", F64: "<f8"}
PIECE_BYTES = 512 << 10
LDS_STEP = 128  # records up to this length are staged through LDS


def piece_records(step):
    """records per piece of a message (include/kicp.h, "ingest_piece_records")"""
    return max(256, PIECE_BYTES // step // 256 * 256)


class Layout:
    def __init__(self, name, step, x, y, z, stamp, t, aligned):
        self.name, self.step, self.x, self.y, self.z, self.stamp, self.t, self.aligned = name, step, x, y, z, stamp, t, aligned
        names, fmts, offs = ["x", "y", "z"], ["<f4"] * 3, [x, y, z]
        if stamp:
            names.append("t"), fmts.append(_FMT[stamp]), offs.append(t)
        self.dtype = np.dtype({"names": names, "formats": fmts, "offsets": offs, "itemsize": step})
        self.wide = 1 if step > LDS_STEP else 0
        self.ends_at_step = max(o + np.dtype(f).itemsize for o, f in zip(offs, fmts)) == step

    def args(self, raw, n):
        """the arguments of PreSteps.Ingest / IngestAhead / okicp.ingest"""
        return (raw, n, self.step, self.x, self.y, self.z, self.stamp or 0, self.t)


#          name                    step    x    y    z  stamp    t  aligned
LAYOUTS = [
    Layout("packed16_f32",           16,   0,   4,   8,  F32,   12, 1),
    Layout("packed16_u32",           16,   0,   4,   8,  U32,   12, 1),
    Layout("packed16_none",          16,   0,   4,   8, None,    0, 1),
    Layout("packed16_none_z_last",   16,   0,   4,  12, None,    0, 1),
    Layout("s16_x_at_2",             16,   2,   8,  12, None,    0, 0),   # only offset_x % 4 fails
    Layout("s18_none",               18,   0,   4,   8, None,    0, 0),   # only point_step % 4 fails
    Layout("s18_none_z_last",        18,   0,   4,  14, None,    0, 0),
    Layout("s20_f64_at_12",          20,   0,   4,   8,  F64,   12, 0),   # every 4-byte term holds, the 8-byte terms do not
    Layout("s24_f64_at_16",          24,   0,   4,   8,  F64,   16, 1),
    Layout("s28_f64_at_16",          28,   0,   4,   8,  F64,   16, 0),   # only point_step % 8 fails
    Layout("s28_f64_at_8_z_last",    28,   0,   4,  24,  F64,    8, 0),
    Layout("odd31_f32_last",         31,   7,  13,   1,  F32,   27, 0),
    Layout("ouster48_f64_last",      48,   0,   4,   8,  F64,   40, 1),
    Layout("s127_f32_last",         127,   3,  20,  50,  F32,  123, 0),
    Layout("s128_f64_last",         128,   0,   4,   8,  F64,  120, 1),   # the longest record that goes through LDS
    Layout("s128_f64_last_x_at_1",  128,   1,   5,   9,  F64,  120, 0),
    Layout("s129_f64_last",         129,   0,   4,   8,  F64,  121, 0),   # the shortest record read field by field
    Layout("s129_u32_last",         129,  64,  68, 100,  U32,  125, 0),
    Layout("s132_f32_last",         132,   0,   4,   8,  F32,  128, 1),
    Layout("s144_f64_last",         144,  16,  20,  24,  F64,  136, 1),
    Layout("s256_f64_last",         256,   0,   4,   8,  F64,  248, 1),
    Layout("s2052_f32_last",       2052,   0,   4,   8,  F32, 2048, 1),   # piece_records clamps to 256: one workgroup per launch
]
LAYOUT = {L.name: L for L in LAYOUTS}


# ---- stamp sets: (rng, n) -> n raw stamps as float64 (n >= 8), extrema unique, in no particular order ---------------------------
def _with_extrema(v, lo, hi):
    v[0], v[1] = lo, hi
    return v


def _velodyne(rng, n):  # relative to the scan end
    return _with_extrema(rng.uniform(-0.0999, -0.0001, n), -0.1, 0.0)


def _mixed_sign(rng, n):
    return _with_extrema(rng.uniform(-0.29, 0.29, n), -0.3, 0.3)


def _boundary(rng, n):  # around round(stamp) >= 1e10: .4 stays, .5 rounds up and converts, the double below .5 stays, 1e10 converts
    below = np.nextafter(9_999_999_999.5, 0.0)
    v = rng.choice(np.array([9_999_999_999.4, 9_999_999_999.5, 1e10, 12.0]), n)
    v[:4] = [9_999_999_999.4, 9_999_999_999.5, 1e10, 12.0]
    v[4], v[5] = 0.25, below  # the extrema in seconds: 0.25 and 9 999 999 999.499998
    return v


def _epoch_mix(rng, n):  # absolute stamps, half of the records in nanoseconds and half in seconds
    ns = rng.random(n) < 0.5
    v = np.where(ns, 1.7e18 + rng.uniform(0.0, 1e8, n), 1.7e9 + rng.uniform(0.0, 0.1, n))
    v[0], v[1] = 1.7e9 - 0.001, (1.7e9 + 0.2) * 1e9
    v[2], v[3] = 1.7e18 + 5e7, 1.7e9 + 0.05
    return v


def _ns_f32(rng, n):  # FLOAT32 stamps >= 1e10 (a float32 near 1.7e18 is a multiple of 2^37 ns) mixed with stamps around 3 s
    ns = rng.random(n) < 0.5
    v = np.where(ns, 1.7e18 + rng.uniform(0.0, 1e15, n), rng.uniform(2.5, 3.5, n))
    v[0], v[1] = 2.25, 1.7e18 + 2e15
    v[2], v[3] = 1.7e18, 3.0
    return v


def _u32_full(rng, n):  # never nanoseconds: 4 294 967 295 < 1e10
    return _with_extrema(rng.integers(1, 2**32 - 1, n).astype(np.float64), 0.0, 4294967295.0)


def _constant(value):
    return lambda rng, n: np.full(n, value)


STAMP_SETS = {
    "velodyne": _velodyne, "mixed_sign": _mixed_sign, "boundary": _boundary, "epoch_mix": _epoch_mix, "ns_f32": _ns_f32,
    "u32_full": _u32_full,
    # hi == lo: every normalised stamp is 0/0
    "const_negative": _constant(-0.05), "const_ns": _constant(1.7e18), "const_u32_max": _constant(4294967295.0),
}
SETS_OF = {F32: ["velodyne", "mixed_sign", "ns_f32", "const_negative"],
           F64: ["velodyne", "mixed_sign", "boundary", "epoch_mix", "const_ns"],
           U32: ["u32_full", "const_u32_max"], None: [None]}
CONSTANT_SETS = ("const_negative", "const_ns", "const_u32_max")


def stamp_seconds(t):
    """TimeStampHandler.cpp:60-63,73-78 on doubles: more than 10 integer digits of round(stamp) (half away from zero) -> nanoseconds"""
    t = np.asarray(t, dtype=np.float64)
    rounded = np.floor(t) + (t - np.floor(t) >= 0.5)  # (exact: both operands are multiples of the same power of two)
    return np.where(rounded >= 1e10, t * 1e-9, t)


# ---- where the extrema sit: name -> (n, piece_records) -> (record of the minimum, record of the maximum) or None ----------------
def _p(f, need):
    return lambda n, pr: f(n, pr) if need(n, pr) else None


PLACEMENTS = {
    "first/last": _p(lambda n, pr: (0, n - 1), lambda n, pr: n >= 2),
    "last/first": _p(lambda n, pr: (n - 1, 0), lambda n, pr: n >= 2),
    "tile0_last/tile1_first": _p(lambda n, pr: (255, 256), lambda n, pr: n >= 257),
    "tile1_first/tile0_last": _p(lambda n, pr: (256, 255), lambda n, pr: n >= 257),
    "piece1_first/piece1_last": _p(lambda n, pr: (pr, min(2 * pr, n) - 1), lambda n, pr: n >= pr + 2),
    "piece1_last/piece1_first": _p(lambda n, pr: (min(2 * pr, n) - 1, pr), lambda n, pr: n >= pr + 2),
    # n = k * piece_records + 1: the last piece is one record
    "tail_piece/tile0_last": _p(lambda n, pr: (n - 1, 255), lambda n, pr: n > pr and n % pr == 1),
    "piece1_first/tail_piece": _p(lambda n, pr: (pr, n - 1), lambda n, pr: n > pr + 1 and n % pr == 1),
}


class Message:
    """A built case: the record array, its bytes (a uint8 array that stays alive: look-ahead borrows it) and what is true of it"""

    def __init__(self, case, rec, imin, imax):
        self.case, self.rec, self.n, self.imin, self.imax = case, rec, len(rec), imin, imax
        self.raw = np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()
        self.args = case.layout.args(self.raw, self.n)


class Case:
    """placement: a name of PLACEMENTS, an explicit (record of the minimum, record of the maximum), or None (constant stamps / none);
    invalid: a fifth of the records are invalid points - all-NaN, x = +inf, z = NaN only, (0, 0, 0) - never those of the extrema"""

    def __init__(self, layout, n, stamps=None, placement=None, invalid=False, tag=""):
        self.layout, self.n, self.stamps, self.placement, self.invalid = LAYOUT[layout], n, stamps, placement, invalid
        assert (stamps is None) == (self.layout.stamp is None) and (stamps is None or stamps in SETS_OF[self.layout.stamp])
        where = placement if isinstance(placement, str) else ("at_%d_%d" % placement if placement else "anywhere")
        self.name = "%s-n%d-%s-%s%s" % (layout, n, stamps or "nostamp", where.replace("/", "+"), tag)
        self.piece_records = piece_records(self.layout.step)
        self.aligned, self.wide = self.layout.aligned, self.layout.wide
        self.min_launches = -(-n // self.piece_records)
        assert n * self.layout.step <= 7_000_000

    def extrema_at(self):
        if self.stamps is None or self.stamps in CONSTANT_SETS or self.placement is None:
            return None
        at = PLACEMENTS[self.placement](self.n, self.piece_records) if isinstance(self.placement, str) else self.placement
        assert at is not None and at[0] != at[1] and max(at) < self.n, self.name
        return at

    def __repr__(self):
        return self.name

    def build(self):
        L, n = self.layout, self.n
        rng = np.random.Generator(np.random.PCG64(zlib.crc32(self.name.encode())))
        rec = np.zeros(n, dtype=L.dtype)
        rec.view(np.uint8)[:] = rng.integers(0, 256, n * L.step, dtype=np.uint8)  # junk in the padding / other fields
        for k in "xyz":
            rec[k] = rng.uniform(-80, 80, n).astype(np.float32)
        at = self.extrema_at()
        if L.stamp:
            assert n >= 8
            raw = STAMP_SETS[self.stamps](rng, n)
            raw = raw[rng.permutation(n)]
            assert np.all(np.isfinite(raw)) and raw.min() > -0.5 and raw.max() < 1.8e19  # the condition on stamps
            t = raw.astype(L.dtype.fields["t"][0])  # (UINT32 sets hold integers, FLOAT32 sets round to nearest)
            assert np.all(np.isfinite(t.astype(np.float64))) and t.astype(np.float64).min() > -0.5 and t.astype(np.float64).max() < 1.8e19
            if at is not None:
                for target, pick in ((at[0], np.argmin), (at[1], np.argmax)):  # the extrema IN SECONDS go where the case names them
                    k = int(pick(stamp_seconds(t.astype(np.float64))))
                    t[[k, target]] = t[[target, k]]
                sec = stamp_seconds(t.astype(np.float64))
                assert (sec == sec.min()).sum() == 1 and (sec == sec.max()).sum() == 1, self.name
            rec["t"] = t
        if self.invalid:
            keep = np.ones(n, dtype=bool)
            if at is not None:
                keep[list(at)] = False
            bad = rng.permutation(np.flatnonzero(keep))[:n // 20 * 4].reshape(4, -1)
            nan, inf = np.float32(np.nan), np.float32(np.inf)
            rec["x"][bad[0]], rec["y"][bad[0]], rec["z"][bad[0]] = nan, nan, nan
            rec["x"][bad[1]] = inf
            rec["z"][bad[2]] = nan
            rec["x"][bad[3]], rec["y"][bad[3]], rec["z"][bad[3]] = 0.0, 0.0, 0.0
        return Message(self, rec, *(at if at is not None else (None, None)))


def numpy_decode(rec, stamp):
    """An independent decode with numpy's structured dtypes: (xyz fp64, normalised stamps or None, (min, max) in seconds)"""
    xyz = np.stack([rec["x"].astype(np.float64), rec["y"].astype(np.float64), rec["z"].astype(np.float64)], axis=1)
    if not stamp or len(rec) == 0:
        return xyz, None, (0.0, 0.0)
    t = stamp_seconds(rec["t"].astype(np.float64))
    lo, hi = t.min(), t.max()
    with np.errstate(invalid="ignore"):
        return xyz, (t - lo) / (hi - lo), (float(lo), float(hi))


def assert_same_cloud(got, want):
    """Decoded clouds are equal as bit patterns (signed zeros count) wherever the point is finite; a record with a NaN or an infinite
    coordinate is only required to be non-finite on both sides: the reference multiplies every point by the sensor pose, the
    identity included (RosUtils.cpp:36), which smears a NaN over the point's other coordinates, and the crop drops it either way"""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape
    finite = np.all(np.isfinite(want), axis=1)
    np.testing.assert_array_equal(got[finite].view(np.uint64), want[finite].view(np.uint64))
    assert not np.all(np.isfinite(got[~finite]), axis=1).any()
    return finite


def sizes_of(layout):
    pr = piece_records(LAYOUT[layout].step)
    sizes = {255, 256, 512, pr - 1, pr, pr + 1, 2 * pr + 1}
    if LAYOUT[layout].step == 2052:
        sizes |= {1000, 3000}  # 4 and 12 single-workgroup launches, alternating between the two streams
    return sorted(sizes)


def _sweep():
    """every layout at every size; the stamp sets of its type and the placements that exist at that size take turns"""
    cases, turn = [], 0
    for L in LAYOUTS:
        pr = piece_records(L.step)
        for n in sizes_of(L.name):
            stamps = SETS_OF[L.stamp][turn % len(SETS_OF[L.stamp])]
            fits = [name for name, f in PLACEMENTS.items() if f(n, pr) is not None]
            cases.append(Case(L.name, n, stamps, fits[turn % len(fits)] if stamps and stamps not in CONSTANT_SETS else None))
            turn += 1
    return cases


def _cross():
    """every non-constant stamp set at every placement, on two pieces and a one-record tail piece of the short aligned / unaligned layouts"""
    cases = []
    for layouts in (["packed16_f32"], ["s24_f64_at_16", "s20_f64_at_12"], ["packed16_u32"]):
        k = 0
        for stamps in SETS_OF[LAYOUT[layouts[0]].stamp]:
            if stamps in CONSTANT_SETS:
                continue
            for placement in PLACEMENTS:
                L = layouts[k % len(layouts)]
                cases.append(Case(L, 2 * piece_records(LAYOUT[L].step) + 1, stamps, placement, tag="-cross"))
                k += 1
    return cases


# look-ahead messages: a launch has at most 48 workgroups, so that a piece of more than 48 tiles is walked in rounds; the extrema sit
# in tiles of piece 0 that are visited on the second and on the third round (the GPU test checks the tile indices against the
# workgroup count of the counters).  The first one opens the sequence as an ordinary message.
AHEAD_CASES = [
    Case("packed16_f32", 50_000, "mixed_sign", "piece1_first/piece1_last", tag="-opener"),
    Case("s132_f32_last", 13_001, "velodyne", "piece1_last/piece1_first", tag="-ahead"),          # wide: 4 pieces of 15 tiles
    Case("s20_f64_at_12", 30_001, "epoch_mix", (50 * 256 + 7, 101 * 256 + 200), tag="-ahead"),      # piece 0: 102 tiles
    Case("packed16_f32", 41_000, "velodyne", (100 * 256 + 5, 60 * 256 + 250), tag="-ahead"),        # piece 0: 128 tiles
]
POSE_CASE = Case("s129_f64_last", piece_records(129) + 1, "epoch_mix", "tail_piece/tile0_last", tag="-pose")

# ---- the consumers of the raw stamps and of invalid points (Preprocess, the chained Frame) ------------------------------------
MAX_RANGE, VOXEL_A, VOXEL_B = 60.0, 0.5, 1.5
STAMP_CONSUMER_CASES = [
    Case("packed16_f32", 20_001, "velodyne", "tile1_first/tile0_last", tag="-consumer"),
    Case("s20_f64_at_12", 20_001, "epoch_mix", "last/first", tag="-consumer"),
]
STAMP_CONSUMER_MIN_RANGE = 1.0
INVALID_CASE = Case("packed16_f32", 3000, "velodyne", "tile0_last/tile1_first", invalid=True, tag="-invalid")
INVALID_MIN_RANGES = (0.0, 1.0)


def prestep_poses():
    """(relative motion of the scan, sensor-to-base pose) of the pre-step cases"""
    from kinematic_icp_amd import synthetic as syn
    return syn.planar_pose(0.4, 0.01, np.deg2rad(3.0)), syn.planar_pose(0.2, 0.0, 0.05, 0.7)


def prestep_runs():
    """(case, deskew, min_range) of every pre-step run of the GPU tests"""
    runs = [(c, d, STAMP_CONSUMER_MIN_RANGE) for c in STAMP_CONSUMER_CASES for d in (False, True)]
    return runs + [(INVALID_CASE, d, m) for d in (False, True) for m in INVALID_MIN_RANGES]


DECODE_CASES = _sweep() + _cross() + AHEAD_CASES + [POSE_CASE] + STAMP_CONSUMER_CASES + [INVALID_CASE]
assert len({c.name for c in DECODE_CASES}) == len(DECODE_CASES)
