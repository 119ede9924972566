"""The case table of the chained pre-steps' regime tests, shared by tests/test_prestep_cases.py (CPU: the premises of every case,
from the oracle alone) and tests/test_gpu_presteps_regimes.py (GPU: kicp_pre.hpp k_frame_* / k_downsample_* / k_scan_blocks and
kicp_pre.hip pre_frame_chain).

A frame case is an input cloud whose survivor counts are pinned by construction (the crop's and the first level's always, the
second level's where a regime depends on it), so that the branch it is named after - a
table's bucket count, a tile count, a workgroup count - is a property of the input: identity relative_motion and lidar_to_base, no
deskew; survivors sit in the middle third of 0.5 m voxels of a slab 6 .. 36 m from the sensor, cropped points 90 .. 110 m away,
max_range = 50 and min_range = 1 in between, so no decision is borderline.  Duplicates of a voxel carry different coordinates (a
downsample that kept another than the first one returns other numbers), and every cloud is shuffled.

BUCKETS / tiles restate kicp_table_order.hpp reference_bucket_count and the tile rules of kicp_pre.hip; the GPU tests assert
them against the read-only counters of kicp_pre_get_option."""
import functools

import numpy as np

IDENT = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
MAX_RANGE, MIN_RANGE = 50.0, 1.0
VOXEL_A, VOXEL_B = 0.5, 1.5
TILE = 256                 # points / buckets per workgroup
SCAN_BLOCKS = 4096         # kFusedScanBlocks: grids beyond it take the separate scan kernel; frames beyond it are not fused
SMALL_TABLE_BUCKETS = 512  # replay_tile: tables below 2 * (256 + 32) buckets take the global path
# the slab the survivors live in, in 1.5 m voxels (each holds 27 voxels of 0.5 m): x 6 .. 30 m, y +-19.5 m, z +-4.5 m
_COARSE = np.array([(x, y, z) for x in range(4, 20) for y in range(-13, 13) for z in range(-3, 3)], dtype=np.int64)
_FINE_IN_COARSE = np.array([(x, y, z) for x in range(3) for y in range(3) for z in range(3)], dtype=np.int64)


def buckets(n):
    """tsl::robin_map::reserve(n): ceil(float(n) / 0.5f) rounded up to a power of two, 0 for 0 (reference_bucket_count)"""
    want = int(np.ceil(np.float32(n) / np.float32(0.5)))
    b = 0
    if want > 0:
        b = 1
        while b < want:
            b <<= 1
    return b


def tiles(count):
    return -(-count // TILE)


def table_tiles(n):
    """256-bucket tiles of the table of n points, as the kernels count them ((mask >> 8) + 1; 0 without a point)"""
    return ((buckets(n) - 1) >> 8) + 1 if n else 0


def l2_workgroups(n_in, previous_n1):
    """workgroups of the second level's launches (kicp_pre.hip): a fresh handle (previous_n1 None) takes up to 1 024, a later
    frame twice the previous frame's second-table tiles (a frame without level-1 survivors counts as one tile), 32 at least"""
    sgrid = tiles(buckets(n_in))
    if previous_n1 is None:
        return min(sgrid, 1024)
    return min(sgrid, max(32, 2 * (tiles(buckets(previous_n1)) if previous_n1 else 1)))


def _slab_voxels(rng, n):
    """n distinct 0.5 m voxels of the slab, in random order"""
    pick = rng.choice(len(_COARSE) * 27, n, replace=False)
    return 3 * _COARSE[pick // 27] + _FINE_IN_COARSE[pick % 27]


def _one_voxel(rng, n):
    return np.array([[21, -5, 2]], dtype=np.int64)


class FrameCase:
    """n_in points of which n0 survive the crop, in n1 voxels of 0.5 m (`voxels`: which) that lie in n2 voxels of 1.5 m (None: not
    pinned - no regime depends on it; it is then counted from the cloud by numpy_counts).
    guess: what the test sets the fused chain's guess to before the frame (None: the handle's own)."""

    def __init__(self, name, n_in, n0, n1, n2=None, guess=None, voxels=_slab_voxels, seed=0):
        self.name, self.n_in, self.n0, self.n1, self.pinned_n2, self.guess, self.voxels, self.seed = name, n_in, n0, n1, n2, guess, voxels, seed
        self.max_range, self.min_range, self.voxel_a, self.voxel_b = MAX_RANGE, MIN_RANGE, VOXEL_A, VOXEL_B

    def __repr__(self):
        return self.name

    @property
    def n2(self):
        if self.pinned_n2 is not None:
            return self.pinned_n2
        return numpy_counts(self.build(), self.max_range, self.min_range, self.voxel_a, self.voxel_b)[2]

    @property
    def counts(self):
        return [self.n0, self.n1, self.n2]

    def build(self):
        return _build_frame(self)

    # ---- what the counts imply (asserted against the oracle on the CPU, against the device's counters on the GPU) ----
    def spec_buckets(self):
        """the first table as the fused chain sizes it: from the guess, the input count where there is none"""
        return buckets(min(self.n_in, self.guess) if self.guess else self.n_in)

    @property
    def hit(self):
        return self.n0 == 0 or self.spec_buckets() == buckets(self.n0)

    @property
    def point_tiles(self):
        return tiles(self.n_in)

    @property
    def l1_tiles(self):
        return ((self.spec_buckets() - 1) >> 8) + 1

    @property
    def l2_tiles(self):
        return table_tiles(self.n1) if self.hit else 0


@functools.lru_cache(maxsize=None)
def _build_frame(case):
    rng = np.random.Generator(np.random.PCG64(1000 + case.seed))
    vox = case.voxels(rng, case.n1)
    assert len(vox) == case.n1 and case.n1 <= case.n0 <= case.n_in and (case.n1 > 0) == (case.n0 > 0)
    owner = np.concatenate([np.arange(case.n1), rng.integers(0, max(case.n1, 1), case.n0 - case.n1)])  # every voxel once, then duplicates
    kept = (vox[owner] + 0.5 + rng.uniform(-1.0 / 6, 1.0 / 6, (case.n0, 3))) * VOXEL_A if case.n0 else np.zeros((0, 3))
    d = rng.normal(size=(case.n_in - case.n0, 3))
    cropped = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(90.0, 110.0, (len(d), 1))
    pts = np.concatenate([kept, cropped])[rng.permutation(case.n_in)]
    pts.setflags(write=False)
    return pts


def _chain_of(okicp, pts, max_range, min_range, voxel_a, voxel_b):
    b0 = okicp.se3_act(IDENT, okicp.preprocess(pts, None, IDENT, max_range, min_range, False))
    b1 = okicp.voxel_downsample(b0, voxel_a) if len(b0) else np.zeros((0, 3))
    b2 = okicp.voxel_downsample(b1, voxel_b) if len(b1) else np.zeros((0, 3))
    for b in (b0, b1, b2):
        b.setflags(write=False)
    return b0, b1, b2


@functools.lru_cache(maxsize=None)
def oracle_chain(case):
    """(buffer 0, 1, 2) of the oracle for a FrameCase or the big frame: computed once per process, shared, read-only"""
    from oracle import okicp
    return _chain_of(okicp, case.build(), case.max_range, case.min_range, case.voxel_a, case.voxel_b)


def numpy_counts(pts, max_range, min_range, voxel_a, voxel_b):
    """the three survivor counts by plain set arithmetic (no hash table): crop, first point per 0.5 voxel, distinct 1.5 voxels"""
    def key(p, v):
        k = np.floor(p / v).astype(np.int64) + (1 << 20)
        return (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]
    r = np.sqrt((pts * pts).sum(axis=1))
    p0 = pts[(r < max_range) & (r > min_range)]
    if not len(p0):
        return [0, 0, 0]
    _, first = np.unique(key(p0, voxel_a), return_index=True)
    p1 = p0[np.sort(first)]
    return [len(p0), len(p1), len(np.unique(key(p1, voxel_b)))]


def F(*a, **k):
    return FrameCase(*a, **k)


# ---- the regimes -----------------------------------------------------------------------------------------------------------------
ORDINARY = F("ordinary_300", 300, 250, 200, guess=250, seed=1)   # frame 1 of the sequences; what a handle must still do after an error
# second level: 64 tiles walked by the 32 workgroups a 300-point frame leaves behind (two turns of the tile loops)
L2_SEVERAL_TILES = F("l2_64_tiles_after_300", 20000, 12000, 6000, guess=12000, seed=2)
# second level: 512 workgroups for one tile / for none; nothing cropped: 157 point tiles under 512 table tiles
ONE_VOXEL = F("one_voxel_40000", 40000, 40000, 1, 1, voxels=_one_voxel, seed=3)
EMPTIED = F("crop_empties_40000", 40000, 0, 0, 0, seed=4)
UNCROPPED = F("nothing_cropped_40000", 40000, 40000, 15000, seed=5)
# more point tiles than table tiles with a right guess: 157 against 8
FEW_SURVIVE = F("1000_of_40000_survive", 40000, 1000, 1000, guess=1000, seed=6)
TILE_CASES = [ONE_VOXEL, EMPTIED, UNCROPPED, FEW_SURVIVE]
# tables of at most 512 buckets (n0 <= 256: the small path of replay_tile at both levels) and the first window table (257)
SMALL_COUNTS = (1, 2, 127, 128, 129, 255, 256, 257)
SMALL_CASES = [F("n0_%d_of_300" % n, 300, n, n, guess=n, seed=10 + k) for k, n in enumerate(SMALL_COUNTS)]
# table A through the window (5 000 points: 16 384 buckets), table B small (their 200 voxels: 512 buckets)
SMALL_B = F("window_a_small_b", 6000, 5000, 200, guess=5000, seed=20)
# a count of 2^k keeps 2^(k+1) buckets, 2^k + 1 takes 2^(k+2): all four (count, guess) pairs around 4 096 and around 256
EDGE_CASES = [F("n0_%d_guess_%d" % (n0, g), n_in, n0, n0, guess=g, seed=30 + n0 % 7)
              for n_in, pair in ((6000, (4096, 4097)), (300, (256, 257))) for n0 in pair for g in pair]
# a table of two buckets for 20 000 voxels: every claim gives up (kClaimProbeLimit); then the right guess for
# ANOTHER cloud of the same counts (the same cloud would find its own points still in the buffers, whatever the second frame wrote)
HOPELESS = F("guess_1_for_20000", 20000, 20000, 20000, guess=1, seed=40)
HOPELESS_THEN_RIGHT = F("guess_20000_for_20000", 20000, 20000, 20000, guess=20000, seed=41)
GROWTH_MIDDLE = F("growth_40000", 40000, 30000, 12000, guess=30000, seed=50)
FRAME_CASES = [ORDINARY, L2_SEVERAL_TILES] + TILE_CASES + SMALL_CASES + [SMALL_B] + EDGE_CASES + [HOPELESS, HOPELESS_THEN_RIGHT, GROWTH_MIDDLE]


# ---- beyond 4 096 workgroups -----------------------------------------------------------------------------------------------------
class BigFrame:
    """1 048 577 points (4 097 point tiles) uniform in +-200 x +-200 x +-2 m: about a tenth of them share their 0.5 m voxel with an
    earlier one, max_range = 150 crops more than half.  Points within 1e-6 m of either range bound are moved inwards (the only
    borderline decision a uniform cloud has; voxel faces are decided by one correctly rounded division on either side)."""
    name = "big_1048577"
    n_in = 1048577
    guess = None
    max_range, min_range, voxel_a, voxel_b = 150.0, 1.0, VOXEL_A, VOXEL_B

    def __repr__(self):
        return self.name

    def build(self):
        return _build_big()


@functools.lru_cache(maxsize=None)
def _build_big():
    rng = np.random.Generator(np.random.PCG64(77))
    pts = rng.uniform(-1.0, 1.0, (BigFrame.n_in, 3)) * np.array([200.0, 200.0, 2.0])
    r = np.sqrt((pts * pts).sum(axis=1))
    near = (np.abs(r - BigFrame.max_range) < 1e-6) | (np.abs(r - BigFrame.min_range) < 1e-6)
    pts[near] *= 0.99
    pts.setflags(write=False)
    return pts


BIG = BigFrame()
# the stand-alone downsample takes the separate scan above 4 096 table tiles = 1 048 576 buckets = 524 288 points
VD_LAST_FUSED, VD_FIRST_SCANNED = 524288, 524289


@functools.lru_cache(maxsize=None)
def oracle_downsample_of_big_prefix(n):
    from oracle import okicp
    out = okicp.voxel_downsample(BIG.build()[:n], VOXEL_A)
    out.setflags(write=False)
    return out


# ---- range errors ----------------------------------------------------------------------------------------------------------------
RANGE_N = 200            # points of a range-error cloud (four waves)
TWIN_VOXEL = (5, 0, 0)   # the issue's example: [2.6, .1, .1] and its twin (5 + 2^21 + .2) * .5
FAR_RANGE = 1e9          # max_range of the range-error frames: nothing is cropped


def _filler(rng, n):
    return (_slab_voxels(rng, n) + 0.5 + rng.uniform(-1.0 / 6, 1.0 / 6, (n, 3))) * VOXEL_A


def twin_cloud(axis, sign, k):
    """RANGE_N points; point k lies in voxel TWIN_VOXEL, point k + 1 in the voxel 2^21 further along `axis`, whose coordinates
    pack_voxel21 masks to the same key; the others lie in the slab"""
    pts = _filler(np.random.Generator(np.random.PCG64(200 + 10 * axis + k)), RANGE_N)
    v = np.array(TWIN_VOXEL, dtype=np.float64)
    pts[k] = (v + np.array([0.2, 0.2, 0.2])) * VOXEL_A
    v[axis] += sign * float(1 << 21)
    pts[k + 1] = (v + np.array([0.4, 0.2, 0.2])) * VOXEL_A
    return pts


TWIN_CASES = [(axis, sign, k) for k in (10, 63) for axis in (0, 1, 2) for sign in (1, -1)]  # k + 1 = 11: mid-wave; 64: first of its wave
LEVEL_B_VOXEL = 1e-4     # 150 m / 1e-4 m = 1.5e6 > 2^20: the second level alone leaves the range


def level_b_cloud():
    """RANGE_N points 150 m out, one per 0.5 m voxel: in range at VOXEL_A, out of range at LEVEL_B_VOXEL"""
    rng = np.random.Generator(np.random.PCG64(300))
    v = np.stack([np.full(RANGE_N, 300), np.arange(RANGE_N) - 100, rng.integers(-4, 4, RANGE_N)], 1)
    return (v + 0.5 + rng.uniform(-1.0 / 6, 1.0 / 6, (RANGE_N, 3))) * VOXEL_A


NONFINITE = (np.nan, np.inf, -np.inf)


def nonfinite_cloud(value, axis, k):
    pts = _filler(np.random.Generator(np.random.PCG64(400 + axis)), RANGE_N)
    pts[k, axis] = value
    return pts
