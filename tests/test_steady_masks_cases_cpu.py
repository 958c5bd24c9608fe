"""tests/test_gpu_steady_masks.py's cases on the CPU oracle alone: they reach what the steady instance's mask pass
(own idle units and vacated cells in one list of quads) has to get right, on steps that instance runs,
so the GPU comparison cannot pass vacuously.  Same map, game seed, Philox policy, injected states and step counts as
the GPU test (tests/steady_masks_cases.py)."""
import json

import pytest

from tests import steady_masks_cases as C


@pytest.mark.parametrize("event", list(C.EVENTS))
def test_the_cases_reach_every_event(event):
    counts = {n: C.census(n)[event] for n in C.CASES}
    print(event, counts)
    assert sum(counts.values()) >= 1, f"no case reaches: {C.EVENTS[event]}"


def test_each_case_reaches_what_it_is_there_for():
    got = {n: C.census(n) for n in C.CASES}
    print(got)
    assert all(g["errors"] == 0 for g in got.values())
    c = got["crowd"]
    assert c["idle_gt16"] >= C.GAMES and c["list_gt12"] >= C.GAMES and c["list_straddles"] >= 1 and c["list_gt32"] >= 1
    r = got["ranged"]
    assert r["ranged_left"] >= 1 and r["ranged_top"] >= 1 and r["ranged_none_after_some"] >= 1
    a = got["afford"]
    assert a["afford_up"] >= 1 and a["afford_down"] >= 1
    e = got["resets"]
    assert e["gameover_inside"] >= 1 and e["gameover_end0"] >= 1 and e["gameover_end1"] >= 1
    assert e["timeout_inside"] >= 1 and e["timeout_end0"] >= 1 and e["timeout_end1"] >= 1
    assert e["reset_list_long"] >= C.GAMES  # every game's first reset
    o = got["over64"]
    assert o["above64"] >= C.GAMES and o["back_from_above64"] >= C.GAMES
    assert o["idle_gt16"] >= 1, "no long list on a steady step after the steps above 64 units"


def test_records_at_every_alignment():
    """A record starts 79 (slot * 256 + cell) bytes into the buffer: live and zero records at cells with every
    c mod 4, in both slots, hit every head / tail byte form of the record stores."""
    every = [(s, k) for s in range(2) for k in range(4)]
    live = sorted(set().union(*(C.census(n)["live"] for n in C.CASES)))
    zero = sorted(set().union(*(C.census(n)["zero"] for n in C.CASES)))
    assert live == every and zero == every, (live, zero)


def test_injected_states_hold_their_features():
    for g in range(C.GAMES):
        for kind in C.CASES:
            d = json.loads(C.injected(kind, g))
            units = d["pgs"]["units"]
            assert len({(u["x"], u["y"]) for u in units}) == len(units) and [u["ID"] for u in units] == list(range(len(units)))
            assert len({a["ID"] for a in d["actions"]}) == len(d["actions"]) and d["time"] == C.T0
        d = json.loads(C.crowd_state(g))
        assert sum(u["type"] == "Barracks" for u in d["pgs"]["units"]) == 4 + 2 * g
        assert sum(u["type"] == "Worker" for u in d["pgs"]["units"]) == 18
        d = json.loads(C.over64_state(g))
        assert len(d["pgs"]["units"]) == 64
        d = json.loads(C.resets_state(g))
        p1 = [u for u in d["pgs"]["units"] if u["player"] == 1]
        assert len(p1) == 1 and p1[0]["type"] == "Base" and p1[0]["hitpoints"] == 1
        d = json.loads(C.ranged_state(g))
        at = {(u["x"], u["y"]): u for u in d["pgs"]["units"]}
        assert at[(0, 5)]["type"] == "Ranged" and at[(3, 5)]["player"] == 1 and at[(3, 6)]["player"] == 1
        assert at[(6, 0)]["type"] == "Ranged" and at[(6, 3)]["player"] == 0 and at[(7, 3)]["player"] == 0
