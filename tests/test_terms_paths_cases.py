"""tests/terms_paths_cases.py without a GPU: every scene enters the regime it was built for (premises(): the oracle's picks, which
queries have a term of 2^22 or more, waves that diverge), and the oracle's sums of a pass equal the sums formed from integers bit for
bit - the reference of tests/test_gpu_terms_paths.py carries no rounding of its own."""
import numpy as np
import pytest

import terms_paths_cases as tc
from checkers import okicp


@pytest.fixture(scope="module")
def omap():
    return tc.oracle_map()


@pytest.mark.parametrize("name", sorted(tc.BUILDERS))
def test_the_scene_enters_its_regime_and_the_oracles_sums_are_exact(omap, name):
    scene = tc.BUILDERS[name]()
    n_far = tc.premises(scene, omap)
    assert n_far == {"one_lane": 1, "spread_64": 64, "whole_wave": 64, "every_lane": 256, "no_lane": 0, "two_tiles": 128}[name]
    sums, _ = okicp.icp_pass(omap, scene.queries, tc.POSE, tc.TAU)
    assert np.array_equal(sums, tc.exact_sums(scene))
