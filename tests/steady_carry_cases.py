"""The cases of tests/test_gpu_steady_carry.py (the steady 16x16 instance's carried issue index, sampled
actions and outcome) and what each of them reaches on the CPU oracle alone
(tests/test_steady_carry_cases_cpu.py).  Test infrastructure only (a plain helper module).

A case: one 16x16 map in `games` self-play games, game seed GAME_SEED, the suite's Philox policy (SEED), and
the rollout_fused calls' step counts.  The injected case puts the same mid-game state into every game; the
games then differ by their policy streams (slot ids)."""
import functools
import json

import numpy as np

from tests import dumps, oracle_py
from tests.combat_maps import BARRACKS16, MELEE16
from tests.defs import DX, DY, SEED  # noqa: F401  (re-exported)
from tests.defs import MOVE as T_MOVE, PRODUCE as T_PRODUCE
from tests.state_cases import GAME_SEED  # noqa: F401  (re-exported)

MAP16 = "maps/16x16/basesWorkers16x16.xml"
GAMES = 64
# Lower bounds of an assignment's duration in every unit-type table version (rts/units/UnitTypeTable.java:
# the fastest move is Light's 8 cycles, the fastest production Worker's 50): an assignment younger than
# that is unfinished whatever its unit
MIN_MOVE, MIN_PRODUCE = 8, 50

CASES = {
    # ranged and melee kills of units that hold pending MOVEs.  Under the random policy the armies first meet after
    # about 185 steps (the oracle counts no death before), so two more calls follow the (40, 40, 7): 300 steps in all
    "melee": dict(map=MELEE16, max_steps=2000, calls=(40, 40, 7, 113, 100), inject=False, oracle_steps=0),
    # several PRODUCEs per player in flight
    "barracks": dict(map=BARRACKS16, max_steps=2000, calls=(60, 60), inject=False, oracle_steps=0),
    # auto-resets strictly inside a launch (steps 25, 50, 75 of 90): the index is rebuilt mid-launch
    "resets": dict(map=MAP16, max_steps=25, calls=(90,), inject=False, oracle_steps=30),
    # see injected_state
    "injected": dict(map=MAP16, max_steps=2000, calls=(30, 20), inject=True, oracle_steps=30),
}


@functools.lru_cache(maxsize=None)
def injected_state():
    """basesWorkers16x16's start with a fight put into the free middle of the map:

    * a Worker of player 0 at (7, 7) holds a PRODUCE of a Barracks (cost 5, 200 cycles) towards (8, 7) and
      stands next to an idle Heavy of player 1 at (7, 8), which kills it with one hit once the policy picks
      the attack;
    * player 0's Base holds a PRODUCE of a Worker (cost 1) towards a free neighbour cell, so player 0's largest
      pending cost drops from 5 to 1 with the Worker's death while the sum drops from 6 to 1;
    * idle Workers of player 0 at (9, 7) and (8, 6) can be sampled a MOVE into (8, 7), the cell the dead
      Worker had reserved (the Heavy at (7, 8) cannot reach them: not adjacent)."""
    ref = oracle_py.OracleVecClient(2, 0, 2000, [MAP16] * 2, seed=GAME_SEED)
    ref.reset()
    d = json.loads(ref.state_json(0))
    ref.close()
    pgs = d["pgs"]
    W, H = pgs["width"], pgs["height"]
    assert (W, H) == (16, 16) and d["time"] == 0 and not d["actions"]
    taken = {(u["x"], u["y"]) for u in pgs["units"]}
    free = lambda x, y: 0 <= x < W and 0 <= y < H and pgs["terrain"][y * W + x] == "0" and (x, y) not in taken  # noqa: E731
    assert all(free(x, y) for x in range(5, 12) for y in range(5, 11)), "the middle of the map is not free"
    nid = max(u["ID"] for u in pgs["units"]) + 1
    new = [("Worker", 0, 7, 7, 1), ("Heavy", 1, 7, 8, 4), ("Worker", 0, 9, 7, 1), ("Worker", 0, 8, 6, 1)]
    for k, (t, p, x, y, hp) in enumerate(new):
        pgs["units"].append({"type": t, "ID": nid + k, "player": p, "x": x, "y": y, "resources": 0, "hitpoints": hp})
    base = next(u for u in pgs["units"] if u["type"] == "Base" and u["player"] == 0)
    bdir = next(k for k in range(4) if free(base["x"] + DX[k], base["y"] + DY[k]))
    for p in pgs["players"]:
        p["resources"] = 10
    d["actions"] = [{"ID": nid, "time": 0, "action": {"type": T_PRODUCE, "parameter": 1, "unitType": "Barracks"}},
                    {"ID": base["ID"], "time": 0, "action": {"type": T_PRODUCE, "parameter": bdir, "unitType": "Worker"}}]
    return json.dumps(d, separators=(",", ":"))


def call_edges(calls):
    """The first and last step index of every call."""
    out, k = set(), 0
    for n in calls:
        out |= {k, k + n - 1}
        k += n
    return out


def _state(dump):
    """dump -> (time, {(x, y): (type, player)}, [(x, y, action type, parameter, issue time)])"""
    time, _, units, assign = dumps.parse(dump)
    units = units.tolist()
    acts = [(units[u][2], units[u][3], t, par, when) for u, t, par, _x, _y, _ut, when in assign.tolist()]
    return time, {(u[2], u[3]): (u[0], u[1]) for u in units}, acts


def _young(t, when, now):
    """An assignment of type t issued at `when` cannot be ready in the cycle that ends the step from time `now`."""
    return when + (MIN_MOVE if t == T_MOVE else MIN_PRODUCE) > now + 1


@functools.lru_cache(maxsize=None)
def census(name):
    """The case's rollout on the oracle alone -> how often each event happens that the carried state has to get
    right (counted over games and steps):

    a  a unit is removed while it holds a present, unfinished MOVE
    b  the same with a PRODUCE
    c  a PRODUCE completes while its player has another one pending
    d  in a step after the first of a call, two idle units (of either player) are sampled MOVE / PRODUCE rows into
       one cell: the merged issue pass has to fall back
    e  an auto-reset in a step that is neither the first nor the last of a call"""
    c = CASES[name]
    S = 2 * GAMES
    ref = oracle_py.OracleVecClient(S, 0, c["max_steps"], [c["map"]] * S, seed=GAME_SEED)
    ref.reset()
    if c["inject"]:
        for g in range(GAMES):
            ref.set_state_json(2 * g, injected_state())
    edges, firsts = call_edges(c["calls"]), set(np.cumsum((0,) + c["calls"][:-1]).tolist())
    out = dict(a=0, b=0, c=0, d=0, e=0, errors=0)
    pre = [_state(ref.dump(2 * g)) for g in range(GAMES)]
    for step in range(sum(c["calls"])):
        m = ref.get_masks(0)
        acts = np.stack([oracle_py.policy(m[s], SEED, s, step, 0) for s in range(S)])
        if step not in firsts:
            for g in range(GAMES):
                now, units, held = pre[g]
                busy = {(x, y) for x, y, *_ in held}
                seen = set()
                for (x, y), (_t, p) in units.items():
                    if p < 0 or (x, y) in busy:
                        continue
                    row = acts[2 * g + p, y * 16 + x]
                    if row[0] in (T_MOVE, T_PRODUCE):
                        tgt = (x + DX[row[row[0]]], y + DY[row[row[0]]])
                        out["d"] += tgt in seen
                        seen.add(tgt)
        _, _, done = ref.step(acts)
        for g in range(GAMES):
            out["errors"] += int(ref.L.oref_errors(ref.h, 2 * g))
            post = _state(ref.dump(2 * g))
            if done[2 * g]:
                out["e"] += step not in edges
            else:
                now, units, held = pre[g]
                _, units2, held2 = post
                still = {(x, y, t, when) for x, y, t, _par, when in held2}
                for x, y, t, _par, when in held:
                    if t not in (T_MOVE, T_PRODUCE):
                        continue
                    gone = units2.get((x, y)) != units[(x, y)]  # (a unit holding an unfinished assignment stands still)
                    if gone and _young(t, when, now):
                        out["a" if t == T_MOVE else "b"] += 1
                    if t == T_PRODUCE and not gone and (x, y, t, when) not in still:  # completed
                        p = units[(x, y)][1]
                        out["c"] += any(t2 == T_PRODUCE and (x2, y2) != (x, y) and units[(x2, y2)][1] == p and
                                        (x2, y2, t2, w2) in still for x2, y2, t2, _p2, w2 in held)
            pre[g] = post
    ref.close()
    return out
