"""tests/first_round_cases.py without a GPU: every scene enters the regime it was built for (premises(): the oracle's picks, the
kernel's keys as tests/test_margin_model.py re-enacts them, search_params()'s bound and margin), so that tests/test_gpu_first_round.py
tests what it says it tests."""
import numpy as np

import first_round_cases as fc


def test_the_scenes_enter_their_regimes():
    scene = fc.build()
    seen = fc.premises(scene, fc.oracle_map(scene))
    assert set(seen) == {"halo", "across", "beyond", "near", "mixed"}
    empty_own, n = seen["halo"]
    assert 4 * empty_own >= n
    deep = fc.build_deep()
    assert set(fc.premises(deep, fc.oracle_map(deep))) == {"deep"}


def test_the_bound_and_the_margin_are_search_params():
    """tau = 0.5 m at 1 m voxels: margin 6.3e-5 m^2, bound tau^2 (1 + 1e-5) + margin, in units^2 (one unit = 1 / 65536 m)"""
    bound_u, margin_u = fc.search_numbers()
    assert bound_u.dtype == margin_u.dtype == np.float32
    np.testing.assert_allclose(margin_u / fc.UPM ** 2, 6.336e-5, rtol=1e-3)
    np.testing.assert_allclose((bound_u - margin_u) / fc.UPM ** 2, 0.25 * 1.00001, rtol=1e-6)
