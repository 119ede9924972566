"""The case table of the regime tests of the clouds' way back to the host, shared by tests/test_egress_cases.py (CPU: the premises
of every case, from the oracle and the rules restated here alone) and tests/test_gpu_egress_regimes.py (GPU: kicp_pre_egress.hpp
k_push_frame / k_push_frame_f32 / k_narrow_f32, kicp_pre_egress.hip follow_pushed_pieces, kicp_map_pc.hpp k_pc_records and
kicp_map_cloud.hip kicp_map_pointcloud_f32).

The three piece rules are RESTATED from include/kicp.h and the comments of those files, not imported: a frame of n_in input points
goes back in kPushPieces = 8 pieces of ceil(ceil(n_in * rec / 8) / 4096) * 4096 bytes (rec: 24 bytes a point as doubles, 12 as
FLOAT32 records), of which the kernel announces what the n0 survivors fill; the copy worker follows the flags up to the first piece
shorter than that, or through all eight.  The map's `want` records go in pieces of min(65536, max(1024, ceil(ceil(want / 4) /
1024) * 1024)) records through kRecSlots = 4 landing slots, 2 048 records (kPcRoundRecords) per LDS round.

Frame cases are prestep_cases.FrameCase clouds (n_in, n0, n1 pinned by construction; no decision borderline); map scenes are lists
of the update calls to make, each bulk call of at least 4 096 points so that a map with a device runs it there."""
import functools

import numpy as np

import prestep_cases as pc

PUSH_PIECES = 8            # kPushPieces (kicp_pre_shared.hpp)
PUSH_ALIGN = 4096          # a piece is a multiple of the bytes one workgroup stores per sweep
PUSH_SWEEP = 16 * 4096     # bytes one sweep of the default grid (16 workgroups) stores
NARROW_GRID_WORDS = 1024 * 256  # words one turn of k_narrow_f32's grid narrows
MAP_SLOTS = 4              # DeviceMirror::kRecSlots (kicp_internal.hpp)
MAP_ROUND = 2048           # kPcRoundRecords (kicp_map_pc.hpp)
MAP_PIECE_MIN, MAP_PIECE_MAX = 1024, 65536
BULK = 4096                # updates of at least this many points run on the map's device


# ---- the rules, restated -----------------------------------------------------------------------------------------------------------
def frame_piece_bytes(n_in, rec_bytes):
    per_piece = -(-(n_in * rec_bytes) // PUSH_PIECES)
    return -(-per_piece // PUSH_ALIGN) * PUSH_ALIGN


def frame_pieces(n0, n_in, rec_bytes):
    """the eight lengths the push kernel announces for n0 survivors of n_in input points"""
    piece, total = frame_piece_bytes(n_in, rec_bytes), n0 * rec_bytes
    return [min(piece, max(0, total - i * piece)) for i in range(PUSH_PIECES)]


def frame_pieces_followed(n0, n_in, rec_bytes):
    """the flags the copy worker waits for: it stops behind the first piece shorter than the piece size, or after the eighth"""
    piece = frame_piece_bytes(n_in, rec_bytes)
    for i, length in enumerate(frame_pieces(n0, n_in, rec_bytes)):
        if length < piece:
            return i + 1
    return PUSH_PIECES


def map_piece_records(want):
    return min(MAP_PIECE_MAX, max(MAP_PIECE_MIN, -(-(-(-want // MAP_SLOTS)) // 1024) * 1024))


def map_pieces(want):
    return -(-want // map_piece_records(want)) if want else 0


# ---- frame cases -------------------------------------------------------------------------------------------------------------------
class PushCase(pc.FrameCase):
    """a FrameCase named after the regime it enters when it returns as records of rec_bytes; `pieces` is what the kernel must
    announce then and `followed` how many flags the worker waits for, both written out (tests/test_egress_cases.py holds them to
    the rules above)"""

    def __init__(self, rec_bytes, n_in, n0, n1, pieces, followed, n2=None, guess=None, voxels=pc._slab_voxels, seed=0):
        super().__init__("rec%d_%d_of_%d" % (rec_bytes, n0, n_in), n_in, n0, n1, n2=n2, guess=guess, voxels=voxels, seed=seed)
        self.rec_bytes, self.pieces, self.followed = rec_bytes, pieces, followed


def _p(*lengths):
    return list(lengths) + [0] * (PUSH_PIECES - len(lengths))


BIG_PIECE = 69632  # of 44 000 points as FLOAT32 records: more than one 65 536-byte sweep of the grid
PUSH_CASES = [
    PushCase(24, 1365, 170, 100, _p(4080), 1, seed=101),                       # piece 4 096 B, first piece short
    PushCase(24, 1365, 171, 100, _p(4096, 8), 2, seed=102),                    # 8 bytes into piece 1
    PushCase(24, 1365, 512, 200, _p(4096, 4096, 4096), 4, seed=103),           # exactly three pieces: piece 3 announced with length 0
    PushCase(24, 1365, 1365, 200, [4096] * 7 + [4088], 8, seed=104),           # eight pieces, the last 8 bytes short
    PushCase(24, 4096, 4096, 300, [12288] * 8, 8, seed=105),                   # all eight pieces full
    PushCase(24, 4096, 4095, 300, [12288] * 7 + [12264], 8, seed=106),
    PushCase(24, 300, 0, 0, _p(), 1, n2=0, seed=107),                          # no survivors
    PushCase(12, 2730, 1, 1, _p(12), 1, n2=1, seed=108),                       # less than one 16-byte unit
    PushCase(12, 2730, 2, 1, _p(24), 1, n2=1, seed=109),                       # one unit (four doubles across two records) and 8 bytes
    PushCase(12, 2730, 3, 2, _p(36), 1, seed=110),
    PushCase(12, 2730, 4, 2, _p(48), 1, seed=111),                             # three units exactly
    PushCase(12, 2730, 341, 200, _p(4092), 1, seed=112),                       # a three-word tail in piece 0
    PushCase(12, 2730, 342, 200, _p(4096, 8), 2, seed=113),                    # two words into piece 1
    PushCase(12, 2730, 1024, 200, _p(4096, 4096, 4096), 4, seed=114),          # exactly three pieces
    PushCase(12, 8192, 8192, 300, [12288] * 8, 8, seed=115),                   # all eight full
    PushCase(12, 8192, 0, 0, _p(), 1, n2=0, seed=116),
    # three full pieces, then one that is longer than a sweep and ends three words past a unit, in the second sweep
    PushCase(12, 44000, 22909, 400, _p(BIG_PIECE, BIG_PIECE, BIG_PIECE, 66012), 4, seed=117),
]
EXACT_BOUNDARY = [c for c in PUSH_CASES if c.pieces == _p(4096, 4096, 4096)]
ALL_FULL = [c for c in PUSH_CASES if c.pieces == [12288] * 8]
STALE_MAKER = pc.GROWTH_MIDDLE  # a 40 000-point frame first: its flags stay behind, with lengths above every smaller frame's piece
# one handle over time: 300, 44 000, 1 365, 4 096, 300 input points
SEQUENCE = [pc.ORDINARY, PUSH_CASES[16], PUSH_CASES[2], PUSH_CASES[5], pc.ORDINARY]
# ... and the landing area grows: a handle's first frame reserves half as much again and 1 MiB (landing_reserve), so behind a
# 300-point frame (7 200 bytes) the first frame that does not fit is one of more than 1 059 376 bytes - 50 000 points as doubles
LANDING_FIRST, LANDING_GROWS = pc.ORDINARY, pc.FrameCase("landing_grows_50000", 50000, 45000, 3000, seed=119)
# the DMA route behind chain.ready (KICP_PRE_PUSH_WGS=0): pieces from 1 MiB on, one event below
DMA_PIECES = pc.FrameCase("dma_pieces_44032", 44032, 30000, 2000, seed=120)
DMA_ONE_EVENT = pc.ORDINARY


# ---- the keypoints' records (buffer 2) ---------------------------------------------------------------------------------------------
def _one_coarse_voxel(rng, n):
    """n distinct 0.5 m voxels inside one voxel of 1.5 m"""
    return 3 * np.array([10, 2, 1], dtype=np.int64) + pc._FINE_IN_COARSE[rng.permutation(27)[:n]]


KP_NONE = PUSH_CASES[6]                                                              # n2 = 0: the guess cannot miss without a survivor
KP_ONE_HIT = pc.FrameCase("kp_one_guess_20", 300, 20, 9, 1, guess=20, voxels=_one_coarse_voxel, seed=130)
KP_ONE_MISS = pc.FrameCase("kp_one_guess_257", 300, 20, 9, 1, guess=257, voxels=_one_coarse_voxel, seed=130)
KP_HIT, KP_MISS = pc.EDGE_CASES[0], pc.EDGE_CASES[1]                                 # 4 096 survivors, guessed as 4 096 / as 4 097
KEYPOINT_CASES = [KP_NONE, KP_ONE_HIT, KP_ONE_MISS, KP_HIT, KP_MISS]
NARROW_SIZES = (1, 87381, 87382)   # 87 382 points: 262 146 words, the second turn of k_narrow_f32's loop
NARROW_GROW, NARROW_REUSE = 100000, 5


def narrow_points(n, seed=140):
    """n points of many magnitudes, either sign, most of them not representable as floats"""
    rng = np.random.Generator(np.random.PCG64(seed + n))
    return rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-3, 3, (n, 1))


# ---- map scenes --------------------------------------------------------------------------------------------------------------------
class MapScene:
    """a map's parameters and the calls that fill it: ("AddPoints", points) / ("Update", points, origin)"""

    def __init__(self, name, voxel, max_distance, cap, calls, caps=()):
        self.name, self.voxel, self.max_distance, self.cap, self.calls, self.caps = name, voxel, max_distance, cap, calls, caps

    def __repr__(self):
        return self.name

    def drive(self, *maps):
        """every call on every map, in lock step"""
        for name, *args in self.calls:
            for m in maps:
                getattr(m, name)(*args)


def _frozen(a):
    a.setflags(write=False)
    return a


def _distinct_voxel_points(rng, n, lo, hi, voxel=1.0, exclude=()):
    """n points, one in each of n distinct voxels of the box [lo, hi) (in voxels), in the middle half of their voxel"""
    lo, hi = np.asarray(lo), np.asarray(hi)
    dims = hi - lo
    pick = rng.choice(int(np.prod(dims)), n + len(exclude), replace=False)
    vox = np.stack(np.unravel_index(pick, dims), 1) + lo
    keep = np.array([tuple(v) not in exclude for v in vox])
    vox = vox[keep][:n]
    assert len(vox) == n
    return (vox + rng.uniform(0.25, 0.75, (n, 3))) * voxel


DEEP_VOXEL, DEEP_POINTS, DEEP_CAP = (3, 2, 1), 4500, 5000
DEEP_CUTS = (2047, 2048, 2049, 4100)  # caps that end this many records into the deep voxel's run


@functools.lru_cache(maxsize=None)
def deep_bucket():
    """cap 5 000: 4 500 points of one voxel on a lattice of 0.055 m (the map keeps points 1 / sqrt(5000) = 0.0141 m apart) and 600
    points in voxels of their own, in one shuffled update: one lane's run spans three LDS rounds"""
    rng = np.random.Generator(np.random.PCG64(150))
    site = np.stack(np.unravel_index(rng.choice(17 * 17 * 16, DEEP_POINTS, replace=False), (17, 17, 16)), 1)
    deep = np.array(DEEP_VOXEL) + 0.05 + 0.055 * site
    rest = _distinct_voxel_points(rng, 600, (-20, -20, -3), (20, 20, 3), exclude={DEEP_VOXEL})
    pts = np.concatenate([deep, rest])[rng.permutation(DEEP_POINTS + 600)]
    return MapScene("deep_bucket", 1.0, 100.0, DEEP_CAP, [("Update", _frozen(pts), _frozen(np.zeros(3)))])


@functools.lru_cache(maxsize=None)
def few_points(k):
    """cap 1, max_distance 5: 4 096 points 100 m away, then 4 096 points that all lie in k voxels round the origin - the second
    update's pruning leaves exactly k points"""
    rng = np.random.Generator(np.random.PCG64(160 + k))
    far = np.array([100.0, 0.0, 0.0]) + rng.uniform(-3.0, 3.0, (BULK, 3))
    vox = np.array([(0, 0, 0), (1, 0, 0), (0, -1, 0), (-1, 1, 0), (0, 0, 1)][:k])
    near = vox[rng.integers(0, k, BULK)] + rng.uniform(0.25, 0.75, (BULK, 3))
    near[:k] = vox + 0.5  # (every voxel at least once)
    return MapScene("few_points_%d" % k, 1.0, 5.0, 1, [("Update", _frozen(far), _frozen(np.array([100.0, 0.0, 0.0]))),
                                                      ("Update", _frozen(near), _frozen(np.zeros(3)))])


@functools.lru_cache(maxsize=None)
def sparse():
    """40 000 points over 120 x 120 x 4 m, then an update of 4 096 points inside eight voxels at the origin whose pruning keeps
    what lies within 6 m: a few hundred points in a table sized for 40 000"""
    rng = np.random.Generator(np.random.PCG64(170))
    wide = rng.uniform(-1.0, 1.0, (40000, 3)) * np.array([60.0, 60.0, 2.0])
    near = rng.uniform(-1.0, 1.0, (BULK, 3)) * 0.9
    return MapScene("sparse", 1.0, 6.0, 20, [("AddPoints", _frozen(wide)), ("Update", _frozen(near), _frozen(np.zeros(3)))])


PIECE_EDGE_CAPS = (4096, 4097, 262144, 262145)


@functools.lru_cache(maxsize=None)
def piece_edges():
    """two AddPoints of 140 000 points in a box of 120 x 120 x 12 m at voxel 1.0: more than 262 145 points"""
    rng = np.random.Generator(np.random.PCG64(180))
    calls = [("AddPoints", _frozen(rng.uniform([0, 0, 0], [120, 120, 12], (140000, 3)))) for _ in range(2)]
    return MapScene("piece_edges", 1.0, 1e6, 20, calls, caps=PIECE_EDGE_CAPS)


def map_scenes():
    return [deep_bucket()] + [few_points(k) for k in range(1, 6)] + [sparse(), piece_edges()]


@functools.lru_cache(maxsize=None)
def oracle_map_cloud(scene):
    """the oracle map's Pointcloud() after the scene (computed once per process, shared, read-only)"""
    from oracle import okicp
    m = okicp.VoxelHashMap(scene.voxel, scene.max_distance, scene.cap)
    scene.drive(m)
    return _frozen(np.array(m.Pointcloud(), dtype=np.float64).reshape(-1, 3))
