"""tests/test_gpu_steady_cycle.py's cases on the CPU oracle alone: they reach what the steady instance's lane-parallel
MOVE pass and its reward / done stores on change have to get right, so the GPU comparison cannot pass
vacuously.  Same maps, game seed, Philox policy and step counts as the GPU test (tests/steady_cycle_cases.py)."""
import json

import pytest

from tests import steady_cycle_cases as C


@pytest.mark.parametrize("event", list(C.EVENTS))
def test_the_cases_reach_every_event(event):
    counts = {n: C.census(n)[event] for n in C.CASES}
    print(event, counts)
    assert sum(counts.values()) >= 1, f"no case reaches: {C.EVENTS[event]}"


def test_each_case_reaches_what_it_is_there_for():
    got = {n: C.census(n) for n in C.CASES}
    print(got)
    assert all(g["errors"] == 0 for g in got.values())
    w = got["workers"]
    assert w["moves2"] >= 1 and w["move_produce"] >= 1 and w["move_gather"] >= 1
    assert got["melee"]["move_attack"] >= 1 and got["skirmish"]["mover_killed"] >= 1
    orders = {o: sum(g[o] for g in got.values()) for o in C.ORDERS}
    print(orders)
    assert sum(orders.values()) == sum(g["attack_on_mover"] for g in got.values())
    # the injected pairs: both orders and the killed mover in every game, on a step the steady instance runs
    sk = got["skirmish"]
    assert sk["attack_first"] >= C.GAMES and sk["move_first"] >= C.GAMES and sk["mover_killed"] >= C.GAMES
    assert sk["on_first_step"] == 0, "the injected assignments are ready in the single-step launch of the general kernel"
    assert got["resource"]["onto_left_cell"] >= 1
    e = got["endgame"]
    assert e["gameover_inside"] >= 1 and e["gameover_end0"] >= 1 and e["gameover_end1"] >= 1 and e["gameover_end2"] >= 1
    t = got["timeouts"]
    assert t["timeout_end0"] >= C.GAMES and t["timeout_end1"] >= C.GAMES and t["timeout_end2"] >= C.GAMES
    assert t["timeout_inside"] >= 3 * C.GAMES  # steps 50, 75 and 100


def test_injected_states_hold_their_features():
    d = json.loads(C.resource_state())
    at = {(u["x"], u["y"]): u for u in d["pgs"]["units"]}
    assert at[(7, 7)]["type"] == "Resource" and at[(7, 7)]["resources"] == 1
    around = [at[(7 + C.DX[k], 7 + C.DY[k])] for k in range(4)]
    assert all(u["type"] == "Worker" for u in around) and sorted(u["player"] for u in around) == [0, 0, 1, 1]
    d = json.loads(C.endgame_state())
    p1 = [u for u in d["pgs"]["units"] if u["player"] == 1]
    assert len(p1) == 1 and p1[0]["type"] == "Base" and p1[0]["hitpoints"] == 1
    assert next(p for p in d["pgs"]["players"] if p["ID"] == 1)["resources"] == 0
    heavies = [u for u in d["pgs"]["units"] if u["type"] == "Heavy"]
    assert len(heavies) == 1 and heavies[0]["player"] == 0
    assert abs(heavies[0]["x"] - p1[0]["x"]) + abs(heavies[0]["y"] - p1[0]["y"]) == 1
