"""tests/mirror_z_cases.py without a GPU: every scene enters the regimes it was built for (premises(): the oracle's picks against a model
of the buckets - sizes, slots, mirror z 0 and 65 535, emptied and re-used buckets), so that tests/test_gpu_mirror_z.py tests what it
says it tests."""
import pytest

import mirror_z_cases as mc


@pytest.fixture(scope="module")
def wall():
    return mc.wall_render()


@pytest.mark.parametrize("name", sorted(mc.BUILDERS))
def test_the_scene_enters_its_regimes(name, wall):
    scene = mc.BUILDERS[name]()
    states = mc.replay(scene, wall)
    assert set(states) == set(scene.looks.values()) == set(scene.queries)
    seen = mc.premises(scene, states)
    print(name, {k: len(v) for k, v in scene.queries.items()}, seen)
    assert seen


def test_the_scenes_are_small():
    """at most 512 queries and a handful of voxels each"""
    for name, build in mc.BUILDERS.items():
        scene = build()
        assert all(len(q) <= 512 for q in scene.queries.values())
        points = sum(len(step[1]) for step in scene.steps if step[0] == "update")
        assert points <= 200, name
