"""tests/lane_start_cases.py without a GPU: every scene enters the regime it was built for (premises(): the oracle's picks, voxel_coord's
fractions and guards in the kernel's arithmetic, cull_todo's test after a first round), and the oracle registers each of them from the
identity in one iteration, at the identity - so that tests/test_gpu_lane_start.py tests what it says it tests."""
import numpy as np
import pytest

import lane_start_cases as lc
from checkers import okicp


@pytest.mark.parametrize("name", sorted(lc.BUILDERS))
def test_the_scene_enters_its_regime(name):
    scene = lc.BUILDERS[name]()
    omap = lc.oracle_map(scene)
    seen = lc.premises(scene, omap)
    assert seen["n"] in (1, 255, 256, 257, 512)
    want = {"shifts": {"shifts"}, "negative": {"shifts"}, "lend": {"shifts", "lend"}, "single": set()}.get(name, {name})
    assert set(seen) == want | {"n"}
    reg = okicp.KinematicRegistration()
    pose = reg.ComputeRobotMotion(scene.queries, omap, lc.I, lc.I, scene.tau)
    assert np.array_equal(pose, lc.I) and reg.last_stats.iterations == 1


def test_the_sizes_cover_one_query_and_both_sides_of_a_block():
    assert {lc.BUILDERS[name]().n for name in lc.BUILDERS} >= {1, 255, 257}
