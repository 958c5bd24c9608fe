"""Case adequacy for tests/test_gpu_fused_state.py, on the CPU oracle alone (as tests/test_combat_scenarios.py for
the combat scenarios): every case of tests.fused_state_cases still draws random damage inside the compared
launches, still ends games by elimination, the v2 table still reaches the engine, and the injection still puts
a game on another game's state and lets it leave that game's path.  A case that decays (a changed map, seed or
policy stream) fails here instead of passing vacuously on the GPU.  The figures of each run are printed; DESIGN.md
§4 records them."""
import numpy as np
import pytest

from tests import combat_maps as C
from tests import fused_state_cases as F

V3 = [c["id"] for c in F.CASES if c["utt"] == 3]
V2 = [c["id"] for c in F.CASES if c["utt"] == 2]


@pytest.fixture(scope="module")
def reached(tmp_path_factory):
    """case id -> (maps, tests.fused_state_cases.reach of the case), each run once for the module."""
    done = {}

    def get(cid):
        if cid not in done:
            c = F.BY_ID[cid]
            maps = c["maps"](tmp_path_factory.mktemp(cid.replace("-", "_")), c["slots"])
            r = F.reach(c, maps)
            print(cid, "draws", {k: int(v.sum()) for k, v in r["draws"].items()}, "games drawing",
                  int((r["draws"][F.STEPS] > 0).sum()), "dones", r["dones"], "wins", r["wins"], "resets min",
                  int(r["resets"].min()))
            done[cid] = (maps, r)
        return done[cid]

    return get


@pytest.mark.parametrize("cid", V3)
def test_v3_cases_draw_damage_inside_the_launches(cid, reached):
    d = reached(cid)[1]["draws"]
    assert d[220].sum() >= 60, f"{cid}: {int(d[220].sum())} damage draws in {F.STEPS} steps"
    assert (d[220] > 0).sum() >= 10, f"{cid}: only {int((d[220] > 0).sum())} games draw"
    assert d[60].sum() >= 1, f"{cid}: no draw within the first 60 steps (the K = 20 + 40 launches)"


def test_resets_case_draws_after_every_first_reset(reached):
    r = reached("mix16-v3-resets")[1]
    after = int((r["draws"][220] - r["draws"][60]).sum())
    assert after >= 50, f"{after} damage draws after step 60"
    assert (r["resets"] >= 5).all(), f"resets per game {r['resets'].tolist()}"


@pytest.mark.parametrize("cid", sorted(F.ENDINGS))
def test_cases_end_games_by_elimination(cid, reached):
    r = reached(cid)[1]
    dones, wins = F.ENDINGS[cid]
    assert r["dones"] >= dones and r["wins"] >= wins, f"{cid}: {r['dones']} dones, {r['wins']} positive WinLoss rewards"


@pytest.mark.parametrize("cid", V2)
def test_v2_table_reaches_the_engine(cid, reached):
    maps, r = reached(cid)
    v1 = F.reach(F.BY_ID[cid], maps, utt=1)
    differ = sum(not np.array_equal(a, b) for a, b in zip(r["dumps"], v1["dumps"]))
    print(cid, "games whose state at step", F.STEPS, "differs from the v1 run:", differ)
    assert differ >= 1, f"{cid}: every game's state at step {F.STEPS} equals the same run under v1"


def test_headline_map_never_draws():
    """Why the headline maps are not used: Workers and Bases hit for 1 in every table."""
    c = dict(F.BY_ID["mix16-v3"])
    r = F.reach(c, [F.HEADLINE16] * c["slots"])
    assert int(r["draws"][F.STEPS].sum()) == 0, r["draws"][F.STEPS]


def test_uniform_policy_never_draws():
    """Why the uniform forms are not used: the unmasked uniform rows never land an attack on melee8x8Mixed6."""
    c = F.BY_ID["melee8-v3"]
    r = F.reach(c, [C.MELEE8] * c["slots"], uniform=True)
    assert int(r["draws"][F.STEPS].sum()) == 0, r["draws"][F.STEPS]


@pytest.mark.parametrize("cid", F.HOST_CHANGES)
def test_injection_moves_games_onto_their_donors(cid, tmp_path):
    c = F.BY_ID[cid]
    r = F.injection(c, c["maps"](tmp_path, c["slots"]))
    print(cid, "injected games", r["games"], "draws after the injection", r["draws"].tolist())
    assert len(r["games"]) == c["slots"] // 8
    assert all(r["differs_before"]), f"{cid}: an injected game equalled its donor before: {r['differs_before']}"
    assert all(r["equal_after"]), f"{cid}: an injected game differs from its donor after: {r['equal_after']}"
    assert all(r["left_donor"]), f"{cid}: an injected game still walks its donor's path at the end: {r['left_donor']}"
    assert int(r["draws"].sum()) >= F.INJECTED_DRAWS[cid], f"{cid}: {r['draws'].tolist()} draws after the injection"
