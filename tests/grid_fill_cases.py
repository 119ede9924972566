"""Inputs shared by the tests of the fill of a grid's unknown cells from another grid (tests/test_grid_fill_host.py runs the host code
over them, tests/test_gpu_grid_fill.py the kernel): a table of every destination class against every source class with the readout at
each threshold on both of its sides, and random counters at the cell counts where the kernel's lanes, waves and workgroups end.
A CASE is (name, dst uint16 [..., 2], src uint16 [..., 2], (min_observations, free_max, occupied_min)); the expected results come
from tests/elev_rough_ref.py's fill()."""
import numpy as np

# the destination's counters: unknown; obstacles and traversable cells, with counters beyond 1 and at 65 535
TABLE_DST = [(0, 0), (1, 0), (0, 1), (3, 7), (0, 9), (65535, 65535), (0, 65535), (65535, 0)]
# the source's counters and what they read at TABLE_CONFIG = (4, 25, 65): seen = min_observations - 1 (nothing) and = min_observations
# (v = 0: FREE); v = 25 = free_max (FREE) and 26 (nothing); v = 64 = occupied_min - 1 (nothing) and 65 (OCCUPIED); 65 535 in both (v =
# 50: nothing), in one (OCCUPIED, FREE); and never seen
TABLE_SRC = [(0, 3), (0, 4), (1, 3), (26, 74), (64, 36), (65, 35), (65535, 65535), (65535, 0), (0, 65535), (0, 0)]
TABLE_CONFIG = (4, 25, 65)
TABLE_READS = [-1, 0, 25, 26, 64, 65, 50, 100, 0, -1]
# the same table under other thresholds: the source's obstacles never taken; everything seen once taken, one way or the other; only v = 0
TABLE_CONFIGS = [TABLE_CONFIG, (4, 25, 101), (1, 49, 50), (1, 0, 1), (3, 100, 101), (65535, 25, 65), (131070, 50, 51)]


def table():
    """-> (dst, src) uint16 [8, 10, 2]: every TABLE_DST against every TABLE_SRC"""
    dst = np.array(TABLE_DST, dtype=np.uint16)[:, None, :].repeat(len(TABLE_SRC), axis=1)
    src = np.array(TABLE_SRC, dtype=np.uint16)[None, :, :].repeat(len(TABLE_DST), axis=0)
    return np.ascontiguousarray(dst), np.ascontiguousarray(src)


SIZES = [(1,), (63,), (64,), (65,), (257,), (300, 300)]  # a lane, a wave less one, a wave, a wave and one, a workgroup and one, 352 workgroups
RANDOM_CONFIG = (2, 30, 60)


def random_pair(shape, seed):
    """a destination as kicp_elev_to_grid* writes it - (0, 0), (0, 1), (1, 0) - with one cell in ten carrying other counters, and a source
    as a mapping run leaves it: half never seen, the rest with counters up to 12, one cell in twenty saturated"""
    rng = np.random.default_rng(seed)
    dst = np.array([(0, 0), (0, 1), (1, 0)], dtype=np.uint16)[rng.choice(3, shape, p=(0.6, 0.25, 0.15))]
    odd = rng.random(shape) < 0.1
    dst[odd] = rng.integers(0, 9, (int(odd.sum()), 2))
    src = rng.integers(0, 13, shape + (2,)).astype(np.uint16)
    src[rng.random(shape) < 0.5] = 0
    src[rng.random(shape) < 0.05] = (65535, rng.integers(0, 2) * 65535)
    return dst.astype(np.uint16), src


def cases():
    dst, src = table()
    out = [("table_%d_%d_%d" % cfg, dst, src, cfg) for cfg in TABLE_CONFIGS]
    out += [("random_" + "x".join(str(s) for s in shape), *random_pair(shape, 40 + k), RANDOM_CONFIG) for k, shape in enumerate(SIZES)]
    return out
