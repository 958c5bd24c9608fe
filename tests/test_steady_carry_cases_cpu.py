"""tests/test_gpu_steady_carry.py's cases on the CPU oracle alone: they reach what the steady instance's carried
state has to get right, so the GPU comparison cannot pass vacuously.  Same maps, game seed, Philox
policy and step counts as the GPU test (tests/steady_carry_cases.py)."""
import json

import pytest

from tests import steady_carry_cases as C

EVENTS = {
    "a": "a unit is removed while it holds a present, unfinished MOVE",
    "b": "a unit is removed while it holds a present, unfinished PRODUCE",
    "c": "a PRODUCE completes while its player has another one pending",
    "d": "after a call's first step, two idle units are sampled MOVE / PRODUCE rows into one cell",
    "e": "an auto-reset in a step that is neither the first nor the last of a call",
}


@pytest.mark.parametrize("event", list(EVENTS))
def test_the_cases_reach_every_event(event):
    counts = {n: C.census(n)[event] for n in C.CASES}
    print(event, counts)
    assert sum(counts.values()) >= 1, f"no case reaches: {EVENTS[event]}"


def test_each_case_reaches_what_it_is_there_for():
    """melee: kills of moving units; barracks: overlapping productions; resets: resets inside the launch; injected:
    the Worker dies with its PRODUCE pending.  No step makes Java print an error."""
    got = {n: C.census(n) for n in C.CASES}
    print(got)
    assert got["melee"]["a"] >= 1
    assert got["barracks"]["c"] >= 1
    assert got["resets"]["e"] >= 3 * C.GAMES  # steps 25, 50 and 75 of the one call of 90
    assert got["injected"]["b"] >= 1
    assert all(g["errors"] == 0 for g in got.values())
    assert all(g["d"] >= 1 for g in got.values())


def test_injected_state_holds_its_three_features():
    d = json.loads(C.injected_state())
    units = {u["ID"]: u for u in d["pgs"]["units"]}
    at = {(u["x"], u["y"]): u for u in units.values()}
    prods = [(units[a["ID"]], a["action"]) for a in d["actions"] if a["action"]["type"] == C.T_PRODUCE]
    assert sorted(a["unitType"] for _, a in prods) == ["Barracks", "Worker"] and all(u["player"] == 0 for u, _ in prods)
    w, act = next((u, a) for u, a in prods if a["unitType"] == "Barracks")
    assert w["type"] == "Worker" and w["hitpoints"] == 1
    heavy = at[(w["x"], w["y"] + 1)]
    assert heavy["type"] == "Heavy" and heavy["player"] == 1 and heavy["ID"] not in {a["ID"] for a in d["actions"]}
    tgt = (w["x"] + C.DX[act["parameter"]], w["y"] + C.DY[act["parameter"]])
    assert tgt not in at
    movers = [at[c] for c in ((tgt[0] + 1, tgt[1]), (tgt[0], tgt[1] - 1)) if c in at]
    assert movers and all(u["type"] == "Worker" and u["player"] == 0 for u in movers)
    assert all(abs(u["x"] - heavy["x"]) + abs(u["y"] - heavy["y"]) > 1 for u in movers)
