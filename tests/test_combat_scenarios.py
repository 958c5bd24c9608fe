"""Scenario adequacy, on the CPU oracle alone: every rollout scenario of tests/test_gpu_combat.py
(tests.combat_maps.ROLLOUTS) still reaches what it is there for — combat units in the observations,
attack slots of range > 1, combat-unit production, eliminations with both signs of WinLoss — under the
suite's own rollout (game seed 3, policy seed 0x5EEDC0DE, masks of player 0).  A scenario that decays
(a changed map, seed or policy stream) fails here instead of passing vacuously on the GPU.  The
census of the suite's older rollouts, which reach none of this, is in DESIGN.md."""
import pytest

from tests import combat_maps as C
from tests.defs import HEAVY, LIGHT, RANGED


@pytest.mark.parametrize("sc", C.ROLLOUTS, ids=[s["id"] for s in C.ROLLOUTS])
def test_scenario_reaches_its_paths(sc, tmp_path):
    c = C.census(sc["maps"](tmp_path, sc["n_slots"]), n_slots=sc["n_slots"], steps=sc["steps"], partial_obs=sc["po"],
                 utt=sc["utt"], crs=sc["crs"], rfs=C.ALL_RFS, n_bot=sc["n_bot"], players=sc["players"])
    print(sc["id"], {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in c.items() if k != "pairs"},
          {p: c["pairs"].count(p) for p in set(c["pairs"])})
    if sc["kind"] == "melee":
        assert all(c["types"][t + 1] > 0 for t in (LIGHT, HEAVY, RANGED)), c["types"]
        assert c["attack_outer"] >= 40, c["attack_outer"]
    elif sc["kind"] == "barracks":
        assert all(c["produce_types"][t] > 0 for t in (LIGHT, HEAVY, RANGED)), c["produce_types"]
        assert sum(c["types"][t + 1] for t in (LIGHT, HEAVY, RANGED)) > 0, c["types"]
    else:
        assert c["terminal"] >= 8, c["terminal"]
        assert c["pairs"].count((1.0, -1.0)) >= 3 and c["pairs"].count((-1.0, 1.0)) >= 3, c["pairs"]
        assert c["attack_reward"] > 0


def test_skirmish_shows_enemy_combat_units_in_partial_views(tmp_path):
    """The 32x32 partially observable skirmish of the records-exchange test, over that test's 66 steps: the
    views hold enemy Light / Heavy / Ranged units (so sight disks of radius 2 and 3 decide what a record
    shows) and attacks of range > 1 are on offer."""
    c = C.census([C.skirmish32(tmp_path / "skirmish32.xml")] * 16, steps=66, partial_obs=True)
    print({k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in c.items() if k != "pairs"})
    assert all(c["types"][t + 1] > 0 for t in (LIGHT, HEAVY, RANGED)), c["types"]
    assert c["enemy_combat_seen"] >= 100 and c["attack_outer"] >= 40, (c["enemy_combat_seen"], c["attack_outer"])
