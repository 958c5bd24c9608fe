"""The cases of tests/test_gpu_steady_cycle.py (the steady 16x16 instance's lane-parallel MOVE pass and its reward /
done stores on change) and what each of them reaches on the CPU oracle alone
(tests/test_steady_cycle_cases_cpu.py).  Test infrastructure only (a plain helper module).

A case: one 16x16 map in GAMES self-play games, game seed GAME_SEED, the suite's Philox policy (SEED), the
rollout_fused calls' step counts, and optionally one mid-game state put into every game (the games then differ by
their policy streams)."""
import functools
import json

import numpy as np

from tests import dumps, oracle_py
from tests.combat_maps import MELEE16
from tests.defs import ATTACK, BARRACKS, BASE, DX, DY, HARVEST, MOVE, PRODUCE, RESOURCE, RETURN, SEED  # noqa: F401
from tests.state_cases import GAME_SEED  # noqa: F401  (re-exported)

MAP16 = "maps/16x16/basesWorkers16x16.xml"
GAMES = 64

CASES = {
    # the benchmark's map from its start: several MOVEs per cycle, MOVEs next to PRODUCEs, HARVESTs and RETURNs
    "workers": dict(map=MAP16, max_steps=2000, calls=(100, 100), inject=None, oracle_steps=30),
    # the armies meet after about 185 steps: ATTACKs in the cycles of MOVEs (the serial fall-back), movers killed
    "melee": dict(map=MELEE16, max_steps=2000, calls=(150, 100, 50), inject=None, oracle_steps=0),
    # see resource_state: Workers step onto the cell a depleted resource left
    "resource": dict(map=MAP16, max_steps=2000, calls=(60, 40), inject="resource", oracle_steps=30),
    # see skirmish_state: Workers with a MOVE under way are killed, some in the cycle in which the MOVE is ready
    "skirmish": dict(map=MAP16, max_steps=2000, calls=(40, 30), inject="skirmish", oracle_steps=30),
    # see endgame_state: decisive game overs at steps that differ from game to game (the census: steps 5, 6, 8, 30,
    # 31, 34, 35, 53 to 55, 58, 63), under calls that end on such a step, one step after one and two steps after one
    "endgame": dict(map=MAP16, max_steps=2000, calls=(7, 24, 10, 16, 10), inject="endgame", oracle_steps=0),
    # max_steps auto-resets at steps 25, 50, 75 and 100: on a call's last step, one and two steps before a call's
    # end, and strictly inside a call
    "timeouts": dict(map=MAP16, max_steps=25, calls=(25, 26, 26, 30), inject=None, oracle_steps=0),
}


def _start():
    ref = oracle_py.OracleVecClient(2, 0, 2000, [MAP16] * 2, seed=GAME_SEED)
    ref.reset()
    d = json.loads(ref.state_json(0))
    ref.close()
    pgs = d["pgs"]
    assert (pgs["width"], pgs["height"]) == (16, 16) and d["time"] == 0 and not d["actions"]
    return d


def _free(pgs):
    taken = {(u["x"], u["y"]) for u in pgs["units"]}
    W, H = pgs["width"], pgs["height"]
    return lambda x, y: 0 <= x < W and 0 <= y < H and pgs["terrain"][y * W + x] == "0" and (x, y) not in taken


@functools.lru_cache(maxsize=None)
def resource_state():
    """basesWorkers16x16's start with a Resource unit holding ONE resource at (7, 7) in the free middle of the map and
    a Worker on each of its four sides, two of each player: the first HARVEST to complete removes the resource unit,
    a later one finds its cell empty or a Worker on it, and the Workers around it can be sampled a MOVE into it."""
    d = _start()
    pgs = d["pgs"]
    free = _free(pgs)
    assert all(free(x, y) for x in range(5, 11) for y in range(5, 11)), "the middle of the map is not free"
    nid = max(u["ID"] for u in pgs["units"]) + 1
    new = [("Resource", -1, 7, 7, 1, 1), ("Worker", 0, 6, 7, 0, 1), ("Worker", 0, 7, 6, 0, 1), ("Worker", 1, 8, 7, 0, 1),
           ("Worker", 1, 7, 8, 0, 1)]
    for k, (t, p, x, y, r, hp) in enumerate(new):
        pgs["units"].append({"type": t, "ID": nid + k, "player": p, "x": x, "y": y, "resources": r, "hitpoints": hp})
    return json.dumps(d, separators=(",", ":"))


@functools.lru_cache(maxsize=None)
def endgame_state():
    """basesWorkers16x16's start with player 1 reduced to its Base at one hit point and no resources (it cannot
    produce), and a Heavy of player 0 on a free cell next to that Base: the game ends, decisively, a few cycles after
    the policy first picks the attack — at a step that differs from game to game."""
    d = _start()
    pgs = d["pgs"]
    pgs["units"] = [u for u in pgs["units"] if not (u["player"] == 1 and u["type"] != "Base")]
    base = next(u for u in pgs["units"] if u["player"] == 1)
    assert base["type"] == "Base"
    base["hitpoints"] = 1
    free = _free(pgs)
    k = next(k for k in range(4) if free(base["x"] + DX[k], base["y"] + DY[k]))
    nid = max(u["ID"] for u in pgs["units"]) + 1
    pgs["units"].append({"type": "Heavy", "ID": nid, "player": 0, "x": base["x"] + DX[k], "y": base["y"] + DY[k],
                         "resources": 0, "hitpoints": 4})
    for p in pgs["players"]:
        if p["ID"] == 1:
            p["resources"] = 0
    return json.dumps(d, separators=(",", ":"))


@functools.lru_cache(maxsize=None)
def skirmish_state():
    """basesWorkers16x16's start with six pairs of a Worker (one hit point) and an enemy Heavy side by side in the free
    middle of the map, three Workers of each player: a Heavy's ATTACK (5 cycles) kills the Worker, which meanwhile may
    hold a MOVE (10 cycles).  Under the policy such a MOVE was issued before the ATTACK whenever both are ready in one
    cycle, since every unit type's MOVE takes longer than any ATTACK: the Worker has left when the ATTACK executes.
    So the state (at time 10) also holds both sequence orders, ready together at time 12: the top left pair's ATTACK
    (issued at 7) put before its Worker's MOVE (issued at 2), which kills the Worker in the cycle in which its MOVE is
    ready, and the top right pair's MOVE put before the ATTACK.  Time 12 is the cycle of the SECOND step after the
    injection: a handle's first launch after it is a single step of the general kernel (no sampled rows are forwarded
    yet), the steady instance runs from the second step on, and these events have to fall on it (STEADY_ONLY)."""
    d = _start()
    pgs = d["pgs"]
    free = _free(pgs)
    assert all(free(x, y) for x in range(4, 12) for y in range(4, 12)), "the middle of the map is not free"
    nid = max(u["ID"] for u in pgs["units"]) + 1
    new = []
    for y in (5, 7, 9):
        a, b = (5, 6) if y != 7 else (6, 5)
        new += [("Worker", 0, a, y, 1), ("Heavy", 1, b, y, 4), ("Worker", 1, a + 3, y, 1), ("Heavy", 0, b + 3, y, 4)]
    for k, (t, p, x, y, hp) in enumerate(new):
        pgs["units"].append({"type": t, "ID": nid + k, "player": p, "x": x, "y": y, "resources": 0, "hitpoints": hp})
    d["time"] = 10
    up = {"type": MOVE, "parameter": 0}
    d["actions"] = [{"ID": nid + 1, "time": 7, "action": {"type": ATTACK, "x": 5, "y": 5}},
                    {"ID": nid, "time": 2, "action": up},
                    {"ID": nid + 2, "time": 2, "action": up},
                    {"ID": nid + 3, "time": 7, "action": {"type": ATTACK, "x": 8, "y": 5}}]
    return json.dumps(d, separators=(",", ":"))


def injected(kind):
    return {"resource": resource_state, "endgame": endgame_state, "skirmish": skirmish_state}[kind]()


def call_ends(calls):
    """step index -> steps left in its call after it (0: the call's last step)"""
    out, k = {}, 0
    for n in calls:
        for i in range(n):
            out[k + i] = n - 1 - i
        k += n
    return out


def call_firsts(calls):
    return set(np.cumsum((0,) + tuple(calls)[:-1]).tolist())


def _state(dump):
    """dump -> (time, {(x, y): (type, player)}, [(x, y, action type, parameter, target x, target y, issue time)] in
    issue order)"""
    s = dumps.parse(dump)
    units = s.units.tolist()
    acts = [(units[u][2], units[u][3], t, par, tx, ty, when) for u, t, par, tx, ty, _ut, when in s.assign.tolist()]
    return s.time, {(u[2], u[3]): (u[0], u[1]) for u in units}, acts


EVENTS = {
    "moves2": "two or more MOVEs complete in one cycle of one game",
    "move_produce": "a MOVE and a PRODUCE complete in one cycle of one game",
    "move_gather": "a MOVE and a HARVEST or RETURN complete in one cycle of one game",
    "move_attack": "a MOVE is ready in the cycle in which an ATTACK completes",
    "attack_on_mover": "an ATTACK completes whose target cell holds a unit with a ready MOVE",
    "mover_killed": "a unit is removed in the cycle in which its own MOVE is ready",
    "onto_left_cell": "a MOVE arrives on a cell that a depleted resource or a destroyed building left earlier in the game",
    "gameover_inside": "a decisive game over on a step that is neither the first nor the last of a call",
    "gameover_end0": "a decisive game over on a call's last step",
    "gameover_end1": "a decisive game over one step before a call's last",
    "gameover_end2": "a decisive game over two steps before a call's last",
    "timeout_inside": "a max_steps auto-reset on a step that is neither the first nor the last of a call",
    "timeout_end0": "a max_steps auto-reset on a call's last step",
    "timeout_end1": "a max_steps auto-reset one step before a call's last",
    "timeout_end2": "a max_steps auto-reset two steps before a call's last",
}
# attack_on_mover by issue order (counted too; the oracle need not reach both under the policy)
ORDERS = {
    "attack_first": "... the ATTACK issued before that MOVE",
    "move_first": "... the MOVE issued before that ATTACK",
}
# The events of the serial fall-back and of killed movers are counted on the steps the steady instance runs only: a
# case's step 0 is a single-step launch of the general kernel in every handle (the first launch after the reset or
# the injection forwards no sampled rows), so what happens there says nothing about the steady instance.  Their
# occurrences on step 0 are counted in `on_first_step` instead.
STEADY_ONLY = ("move_attack", "attack_on_mover", "mover_killed", "attack_first", "move_first")


@functools.lru_cache(maxsize=None)
def census(name):
    """The case's rollout on the oracle alone -> how often each of EVENTS happens, over games and steps (and `errors`:
    steps in which Java printed an error; `on_first_step`: see STEADY_ONLY).

    An assignment of the state before a step that the state after it no longer holds left in that step's cycle.  A
    MOVE whose unit then stands on its target cell completed.  Whether a MOVE whose unit is gone was ready is told by
    its duration: every completed MOVE gives its unit type's (issue time to completion), and a removed unit's MOVE
    was ready if the cycle's time is its issue time plus that."""
    c = CASES[name]
    S = 2 * GAMES
    ref = oracle_py.OracleVecClient(S, 0, c["max_steps"], [c["map"]] * S, seed=GAME_SEED)
    ref.reset()
    if c["inject"]:
        for g in range(GAMES):
            ref.set_state_json(2 * g, injected(c["inject"]))
    ends, firsts = call_ends(c["calls"]), call_firsts(c["calls"])
    out = dict.fromkeys(list(EVENTS) + list(ORDERS), 0)
    out["errors"] = out["on_first_step"] = 0

    def count(event, step, k=1):
        assert event in STEADY_ONLY
        out[event if step > 0 else "on_first_step"] += int(k)

    move_time = {}  # unit type -> cycles
    removed = []  # (unit type, issue time, cycle time, attacked: None or "attack_first" / "move_first", step)
    pre = [_state(ref.dump(2 * g)) for g in range(GAMES)]
    left = [set() for _ in range(GAMES)]  # cells a resource or a building has left since the game's start
    for step in range(sum(c["calls"])):
        m = ref.get_masks(0)
        acts = np.stack([oracle_py.policy(m[s], SEED, s, step, 0) for s in range(S)])
        _, rew, done = ref.step(acts)
        for g in range(GAMES):
            out["errors"] += int(ref.L.oref_errors(ref.h, 2 * g))
            post = _state(ref.dump(2 * g))
            if done[2 * g]:
                kind = "gameover" if rew[2 * g] != 0 else "timeout"
                if step not in firsts and ends[step] > 0:
                    out[kind + "_inside"] += 1
                if ends[step] <= 2:
                    out[f"{kind}_end{ends[step]}"] += 1
                left[g] = set()
                pre[g] = post
                continue
            now, units, held = pre[g]
            _, units2, held2 = post
            still = {(x, y, t, when) for x, y, t, _p, _tx, _ty, when in held2}
            over = [(i, a) for i, a in enumerate(held) if (a[0], a[1], a[2], a[6]) not in still and a[2] != 0]
            moved, movers_gone, n = [], [], dict.fromkeys((MOVE, HARVEST, RETURN, PRODUCE, ATTACK), 0)
            for i, (x, y, t, par, tx, ty, when) in over:
                who = units[(x, y)]
                if t == MOVE:
                    to = (x + DX[par], y + DY[par])
                    if units2.get(to) == who and to not in units:
                        moved.append((i, (x, y), to))
                        assert move_time.setdefault(who[0], now + 1 - when) == now + 1 - when, "a unit type's MOVE time varies"
                        n[MOVE] += 1
                    else:
                        movers_gone.append((i, (x, y), who[0], when))
                elif units2.get((x, y)) == who:  # the unit is still there: its assignment completed
                    n[t] += 1
            attacks = [(i, (tx, ty)) for i, (x, y, t, _p, tx, ty, _w) in over if t == ATTACK and units2.get((x, y)) == units[(x, y)]]
            out["moves2"] += n[MOVE] >= 2
            out["move_produce"] += n[MOVE] >= 1 and n[PRODUCE] >= 1
            out["move_gather"] += n[MOVE] >= 1 and n[HARVEST] + n[RETURN] >= 1
            count("move_attack", step, n[MOVE] >= 1 and n[ATTACK] >= 1)
            for i, frm, to in moved:
                out["onto_left_cell"] += to in left[g]
                for j, tgt in attacks:  # (a mover that survived the hit)
                    if tgt == frm:
                        count("attack_on_mover", step)
                        count("attack_first" if j < i else "move_first", step)
            for i, frm, ut, when in movers_gone:
                hit = [j for j, tgt in attacks if tgt == frm]
                removed.append((ut, when, now + 1, None if not hit else "attack_first" if hit[0] < i else "move_first", step))
            for cellxy, (t, _p) in units.items():
                if t in (RESOURCE, BASE, BARRACKS) and cellxy not in units2:
                    left[g].add(cellxy)
            pre[g] = post
    ref.close()
    for ut, when, at, order, step in removed:
        if ut in move_time and when + move_time[ut] == at:
            count("mover_killed", step)
            if order:
                count("attack_on_mover", step)
                count(order, step)
    return out
