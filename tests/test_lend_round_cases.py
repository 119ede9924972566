"""tests/lend_round_cases.py without a GPU: premises() replays the first lending round of every wave and each scene enters the regime
tests/test_gpu_lend_round.py names it for - (busy lanes, idle lanes, jobs offered, jobs lent) per wave and what the lent visits find."""
import pytest

import lend_round_cases as lc

WANT = {  # (busy, idle, offered, lent) of every wave; lent visits that find nothing / the winner / a tie the owner wins / a loser
    "no_idle": ((64, 0, 64, 0), (0, 0, 0, 0)),
    "one_idle_two_voxels": ((63, 1, 2, 1), (0, 0, 0, 1)),         # the one lent visit is +y of the `three` lane
    "more_jobs_than_idle": ((56, 8, 48, 8), (0, 4, 0, 4)),        # four lanes lend both voxels: +y (a loser) and ++0 (the winner)
    "more_than_32_jobs": ((20, 44, 40, 32), (0, 64, 0, 64)),      # kLendJobs caps 40 offers at 32, in each of four waves
    "lent_finds_nothing": ((16, 48, 16, 16), (16, 0, 0, 0)),
    "lent_finds_winner": ((16, 48, 16, 16), (0, 16, 0, 0)),
    "lent_ties": ((16, 48, 16, 16), (0, 0, 16, 0)),
}


@pytest.mark.parametrize("name", sorted(lc.BUILDERS))
def test_the_scene_enters_its_regime(name):
    scene = lc.BUILDERS[name]()
    seen = lc.premises(scene, lc.oracle_map(scene))
    wave, lent = WANT[name]
    assert seen["waves"] == [wave] * (scene.n // 64)
    assert (seen["lent"]["nothing"], seen["lent"]["winner"], seen["lent"]["tie"], seen["lent"]["loser"]) == lent


def test_the_regimes_are_the_seven():
    assert set(WANT) == set(lc.BUILDERS) and len(WANT) == 7
