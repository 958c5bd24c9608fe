"""The cases of tests/test_gpu_steady_masks.py (the steady 16x16 instance's mask pass: own idle units and vacated
cells in one list of quads) and what each of them reaches on the CPU oracle alone
(tests/test_steady_masks_cases_cpu.py).  Test infrastructure only (a plain helper module).

A case: basesWorkers16x16 in GAMES self-play games, game seed GAME_SEED, the suite's Philox policy (SEED), the
rollout_fused calls' step counts, max_steps, and one mid-game state per game (`injected(kind, g)`).  A sampled NONE
ends in the next cycle, so a unit with nothing else to do (a building whose player cannot pay) is idle in every step,
and a mobile unit is idle when its last action ends: the states hold assignments under way that complete on chosen
steps, which is what puts many idle units, many vacated cells or a reset on a chosen step.  Step 0 of a case is a
single-step launch of the general kernel in every handle (nothing is forwarded yet after an injection); the census
counts events on the steps the steady instance runs, 1 and later."""
import functools
import json

import numpy as np

from tests import dumps, oracle_py
from tests.defs import ATTACK, BARRACKS, BASE, DX, DY, NAMES, NONE, PRODUCE, RANGED, RESOURCE, RETURN, SEED, WORKER  # noqa: F401
from tests.defs import COST, HEAVY, HP
from tests.state_cases import GAME_SEED  # noqa: F401  (re-exported)

MAP16 = "maps/16x16/basesWorkers16x16.xml"
GAMES = 8
T0 = 100          # the injected states' time: later than any duration, so every issue time is positive
NONE_TIME = 10    # cycles of the injected NONEs (any value: the issue time is set from the step they complete on)
RETURN_TIME, PRODUCE_WORKER_TIME, HEAVY_ATTACK_TIME = 10, 50, 5  # UnitTypeTable VERSION_ORIGINAL
BUSY = 1000       # the duration of a NONE that keeps a unit out of the way
RANGE = 3         # a Ranged unit's attack range

CASES = {
    # see crowd_state: more than 16 own idle units at once (a second pass of 16 quads), vacated cells that follow
    # fewer than 16 idle units past the pass's end
    "crowd": dict(max_steps=2000, calls=(2, 3, 6, 13, 2, 10), oracle_steps=30),
    # see ranged_state: idle Ranged units at the left and top edges, enemies inside and just outside their range
    "ranged": dict(max_steps=2000, calls=(3, 2, 9, 16, 12), oracle_steps=30),
    # see afford_state: a player's resources cross the Worker's cost upwards (a RETURN) and downwards (a PRODUCE pays)
    # between two consecutive steps with an idle Base
    "afford": dict(max_steps=2000, calls=(2, 5, 3, 10, 20), oracle_steps=30),
    # see resets_state: decisive game overs on steps 3, 4, 6 and 9 and max_steps resets twelve steps after the last
    # reset, under calls that end on such a step, one step after one, and later
    "resets": dict(max_steps=12, calls=(2, 3, 3, 4, 5, 3, 2, 6), oracle_steps=0),
    # see over64_state: 64 units, a 65th produced on the third step, three killed on the sixth
    "over64": dict(max_steps=2000, calls=(2, 3, 2, 3, 12), oracle_steps=0),
}


@functools.lru_cache(maxsize=None)
def _start_text():
    ref = oracle_py.OracleVecClient(2, 0, 2000, [MAP16] * 2, seed=GAME_SEED)
    ref.reset()
    text = ref.state_json(0)
    ref.close()
    return text


def _start():
    """basesWorkers16x16's reset state at time T0, unit IDs = list positions, no actions: Resources at (0, 0), (0, 1),
    (15, 14), (15, 15), Bases at (2, 2) and (13, 13), Workers at (1, 1) and (14, 14), five resources each."""
    d = json.loads(_start_text())
    pgs = d["pgs"]
    assert (pgs["width"], pgs["height"]) == (16, 16) and d["time"] == 0 and not d["actions"] and "1" not in pgs["terrain"]
    assert all(u["y"] < 3 or u["y"] > 12 for u in pgs["units"]), "rows 3..12 are not free"
    d["time"] = T0
    for i, u in enumerate(pgs["units"]):
        u["ID"] = i
    return d


def _add(d, t, player, x, y, resources=0, hp=None):
    pgs = d["pgs"]
    assert 0 <= x < 16 and 0 <= y < 16 and all((u["x"], u["y"]) != (x, y) for u in pgs["units"]), f"({x}, {y}) is taken"
    u = {"type": NAMES[t], "ID": len(pgs["units"]), "player": player, "x": x, "y": y, "resources": resources,
         "hitpoints": HP[t] if hp is None else hp}
    pgs["units"].append(u)
    return u


def _assign(d, u, action, fires_at, eta):
    """u's action under way, completing in the fires_at-th step after the injection (issue time + eta <= time)"""
    assert fires_at >= 1
    d["actions"].append({"ID": u["ID"], "time": d["time"] + fires_at - eta, "action": action})


def _idle_on(d, u, fires_at):
    """u holds a NONE that completes in the fires_at-th step: it is idle when that step writes its masks"""
    _assign(d, u, {"type": NONE, "parameter": NONE_TIME}, fires_at, NONE_TIME)


def _set_resources(d, r0, r1):
    for p, r in zip(d["pgs"]["players"], (r0, r1)):
        p["resources"] = r


def _unit(d, type_name, player):
    return next(u for u in d["pgs"]["units"] if u["type"] == type_name and u["player"] == player)


def _text(d):
    d["actions"].sort(key=lambda a: a["time"])  # (issue order)
    return json.dumps(d, separators=(",", ":"))


def _cells(rows):
    return [(x, y) for y in rows for x in range(16)]


@functools.lru_cache(maxsize=None)
def crowd_state(g):
    """Neither player owns a resource, so a Barracks can only wait: 4 + 2 g of them (owners alternating, on
    consecutive cells: every cell index mod 4, both slots) are idle in every step.  16 Workers, eight of each player,
    spread over the free middle, become idle together on the second step and again whenever their next actions end
    together: 20 + 2 g own idle units in that step (a second pass), and in the step after it the cells of those that
    were given something to do are vacated behind the 4 + 2 g Barracks and the Workers left idle (the list passes a
    pass's end inside the vacated cells in some of the games)."""
    d = _start()
    _set_resources(d, 0, 0)
    cells = iter(_cells(range(4, 6)))
    for k in range(4 + 2 * g):
        x, y = next(cells)
        _idle_on(d, _add(d, BARRACKS, k & 1, x, y), 2)
    for k in range(16):
        _idle_on(d, _add(d, WORKER, k & 1, 1 + 2 * (k % 8) - (k // 8), 8 + 2 * (k // 8)), 2)
    return _text(d)


@functools.lru_cache(maxsize=None)
def ranged_state(g):
    """Ranged units of player 0 on the left edge and of player 1 on the top edge (columns / rows 0 to 2, where the
    attack window's bits shift the other way), each idle first on step 2 + (g + its index) mod 3, with Barracks of
    the other player at distance 3 (inside), sqrt 8 (inside) and sqrt 10 (just outside)."""
    d = _start()
    k = 0
    for x, y in ((0, 5), (1, 9), (2, 12)):
        _idle_on(d, _add(d, RANGED, 0, x, y), 2 + (g + k) % 3)
        k += 1
    for x, y in ((3, 5), (3, 7), (3, 10), (3, 6), (5, 11)):  # (3,5)-(0,5): 3; (3,7)-(1,9): sqrt 8; (3,6)-(0,5): sqrt 10
        _idle_on(d, _add(d, BARRACKS, 1, x, y), 7)
    for x, y in ((6, 0), (10, 1), (13, 2)):
        _idle_on(d, _add(d, RANGED, 1, x, y), 2 + (g + k) % 3)
        k += 1
    for x, y in ((6, 3), (8, 3), (12, 3), (7, 3), (14, 5)):  # (6,3)-(6,0): 3; (8,3)-(10,1): sqrt 8; (7,3)-(6,0): sqrt 10
        _idle_on(d, _add(d, BARRACKS, 0, x, y), 7)
    return _text(d)


@functools.lru_cache(maxsize=None)
def afford_state(g):
    """Neither player owns a resource.  Each has ten more Bases with free cells around them, idle from the second
    step on or later (a Base that cannot pay can only wait, so it is idle in every step), a Worker that carries a
    resource beside its first Base with a RETURN completing on step 3 + g mod 3 (0 -> 1: the Worker becomes affordable)
    and a PRODUCE Worker of its first Base completing on step 6 + g mod 4 (it pays: 1 -> 0)."""
    d = _start()
    _set_resources(d, 0, 0)
    for p, (wx, wy, rdir, pdir) in enumerate(((2, 3, 0, 1), (13, 12, 2, 3))):  # the Worker below / above the Base
        base = _unit(d, "Base", p)
        assert (wx + DX[rdir], wy + DY[rdir]) == (base["x"], base["y"])
        _assign(d, _add(d, WORKER, p, wx, wy, resources=1), {"type": RETURN, "parameter": rdir}, 3 + g % 3, RETURN_TIME)
        _assign(d, base, {"type": PRODUCE, "parameter": pdir, "unitType": NAMES[WORKER]}, 6 + g % 4, PRODUCE_WORKER_TIME)
        for k in range(5):
            b = _add(d, BASE, p, 1 + 3 * k, 5 + 4 * p)
            _idle_on(d, b, 2 + 2 * k)
            b2 = _add(d, BASE, p, 2 + 3 * k, 7 + 4 * p)
            _idle_on(d, b2, 3 + 2 * k)
    return _text(d)


RESET_STEPS = (3, 4, 6, 9)  # the step (from 0) of games 0..3's decisive end


@functools.lru_cache(maxsize=None)
def resets_state(g):
    """Player 1 is its Base alone, at one hit point and without resources.  In games 0..3 a Heavy of player 0 beside it
    holds an ATTACK that completes on step RESET_STEPS[g]: the game ends there; the other games run into max_steps.
    30 Barracks of player 0 (no resources: they can only wait) are idle from the step before the game's first reset
    on, or from the step of it, so that the reset's vacated list is long."""
    d = _start()
    _set_resources(d, 0, 0)
    pgs = d["pgs"]
    pgs["units"] = [u for u in pgs["units"] if not (u["player"] == 1 and u["type"] == "Worker")]
    for i, u in enumerate(pgs["units"]):
        u["ID"] = i
    base = _unit(d, "Base", 1)
    base["hitpoints"] = 1
    _assign(d, base, {"type": NONE, "parameter": BUSY}, BUSY, BUSY)
    heavy = _add(d, HEAVY, 0, base["x"] - 1, base["y"])
    first = RESET_STEPS[g] if g < len(RESET_STEPS) else CASES["resets"]["max_steps"] - 1  # the first reset's step
    if g < len(RESET_STEPS):
        _assign(d, heavy, {"type": ATTACK, "x": base["x"], "y": base["y"]}, first + 1, HEAVY_ATTACK_TIME)
    else:
        _assign(d, heavy, {"type": NONE, "parameter": BUSY}, BUSY, BUSY)
    cells = iter(_cells(range(4, 12)))
    for n, fires_at in ((20, first), (10, first + 1)):
        for k in range(n):
            x, y = next(cells)
            b = _add(d, BARRACKS, 0, x, y)
            if fires_at >= 1:
                _idle_on(d, b, fires_at)
    return _text(d)


@functools.lru_cache(maxsize=None)
def over64_state(g):
    """64 units.  Player 0's Base completes a Worker on the third step (65: that step writes its masks the general way)
    and three Heavies of player 0 kill the Workers of player 1 beside them on the sixth (62).  The rest are Barracks
    of both players without anything to produce from, idle from the second step on or later, and Resources."""
    d = _start()
    _set_resources(d, 1, 0)
    base = _unit(d, "Base", 0)
    _assign(d, base, {"type": PRODUCE, "parameter": 1, "unitType": NAMES[WORKER]}, 3, PRODUCE_WORKER_TIME)
    for k in range(3):
        x = 2 + 4 * k + (g & 1)
        h, w = _add(d, HEAVY, 0, x, 12), _add(d, WORKER, 1, x + 1, 12)
        _assign(d, h, {"type": ATTACK, "x": w["x"], "y": w["y"]}, 6, HEAVY_ATTACK_TIME)
        _assign(d, w, {"type": NONE, "parameter": BUSY}, BUSY, BUSY)
    cells = iter(_cells(range(4, 11)))
    for k in range(40):
        x, y = next(cells)
        _idle_on(d, _add(d, BARRACKS, k & 1, x, y), 2 + (k // 2 + g) % NONE_TIME)
    for k in range(10):
        x, y = next(cells)
        _add(d, RESOURCE, -1, x, y, resources=5)
    assert len(d["pgs"]["units"]) == 64
    return _text(d)


def injected(kind, g):
    return {"crowd": crowd_state, "ranged": ranged_state, "afford": afford_state, "resets": resets_state,
            "over64": over64_state}[kind](g)


def call_ends(calls):
    """step index -> steps left in its call after it (0: the call's last step)"""
    out, k = {}, 0
    for n in calls:
        for i in range(n):
            out[k + i] = n - 1 - i
        k += n
    return out


EVENTS = {
    "idle_gt16": "more than 16 own idle units in one game (a second pass of quads)",
    "list_gt12": "more than 12 own idle units and vacated cells in one game",
    "list_straddles": "at most 16 own idle units, and vacated cells that take the list past 16 entries",
    "list_gt32": "more than 32 own idle units and vacated cells in one game (a third pass)",
    "ranged_left": "an idle Ranged unit in columns 0..2 with an enemy in range and one just outside (distance sqrt 10)",
    "ranged_top": "an idle Ranged unit in rows 0..2 with an enemy in range and one just outside (distance sqrt 10)",
    "ranged_none_after_some": "a step without an idle Ranged unit right after a step with one",
    "afford_up": "a player's idle Bases gain the produce bits between two consecutive steps (its resources reach the cost)",
    "afford_down": "a player's idle Bases lose the produce bits between two consecutive steps (its resources fall below)",
    "gameover_inside": "a decisive game over on a step that is neither the last of its call nor the one before",
    "gameover_end0": "a decisive game over on a call's last step",
    "gameover_end1": "a decisive game over one step before a call's last",
    "timeout_inside": "a max_steps reset on a step that is neither the last of its call nor the one before",
    "timeout_end0": "a max_steps reset on a call's last step",
    "timeout_end1": "a max_steps reset one step before a call's last",
    "reset_list_long": "a reset step that vacates 12 cells or more",
    "above64": "a step that leaves more than 64 units, after a step that left 64 or fewer",
    "back_from_above64": "a step that leaves 64 units or fewer, after a step that left more",
}


def _sources(m):
    """masks [S][H][W][K] -> bool [S][H*W]: the cells with an own idle unit"""
    return m[:, :, :, 0].reshape(m.shape[0], -1) != 0


@functools.lru_cache(maxsize=None)
def census(name):
    """The case's rollout on the oracle alone -> how often each of EVENTS happens on the steps the steady instance runs
    (step 1 and later), over games and steps; `errors`: steps in which Java printed an error; `live` / `zero`: the
    (slot, cell mod 4) pairs at which a record of an own idle unit / of a vacated cell was written.

    Step t writes the masks the oracle holds after it: its own idle units are their source cells, its vacated cells
    the source cells of the masks before it that are none now."""
    c = CASES[name]
    S = 2 * GAMES
    ref = oracle_py.OracleVecClient(S, 0, c["max_steps"], [MAP16] * S, seed=GAME_SEED)
    ref.reset()
    for g in range(GAMES):
        ref.set_state_json(2 * g, injected(name, g))
    ends = call_ends(c["calls"])
    out = dict.fromkeys(EVENTS, 0)
    out["errors"] = 0
    live, zero = set(), set()
    m = ref.get_masks(0).copy()
    prev = dict(src=_sources(m), ranged=[1] * GAMES, nu=[dumps.n_units(ref.dump(2 * g)) for g in range(GAMES)],
                prod=[[None, None] for _ in range(GAMES)])
    for step in range(sum(c["calls"])):
        acts = np.stack([oracle_py.policy(m[s], SEED, s, step, 0) for s in range(S)])
        _, rew, done = ref.step(acts)
        m = ref.get_masks(0).copy()
        src = _sources(m)
        steady = step >= 1
        cur = dict(src=src, ranged=[], nu=[], prod=[])
        for g in range(GAMES):
            out["errors"] += int(ref.L.oref_errors(ref.h, 2 * g))
            st = dumps.parse(ref.dump(2 * g))
            units = st.units.tolist()
            cur["nu"].append(len(units))
            now = np.concatenate([src[2 * g], src[2 * g + 1]])
            gone = np.concatenate([prev["src"][2 * g], prev["src"][2 * g + 1]]) & ~now
            ri, ng = int(now.sum()), int(gone.sum())
            at = {(x, y): (t, p) for t, p, x, y, _hp, _r in units}
            idle_ranged = [(x, y, p) for (x, y), (t, p) in at.items() if t == RANGED and p >= 0 and src[2 * g + p][16 * y + x]]
            cur["ranged"].append(len(idle_ranged))
            prod = [None, None]  # per player: do its idle Bases hold the produce bit (None: no idle Base with a free cell)
            for (x, y), (t, p) in at.items():
                if t == BASE and src[2 * g + p][16 * y + x] and any(
                        0 <= x + DX[k] < 16 and 0 <= y + DY[k] < 16 and (x + DX[k], y + DY[k]) not in at for k in range(4)):
                    prod[p] = bool(m[2 * g + p, y, x, 1 + PRODUCE]) or bool(prod[p])
            cur["prod"].append(prod)
            if not steady:
                continue
            if cur["nu"][g] > 64:  # (the step wrote its masks the general way)
                out["above64"] += prev["nu"][g] <= 64
                continue
            out["back_from_above64"] += prev["nu"][g] > 64
            out["idle_gt16"] += ri > 16
            out["list_gt12"] += ri + ng > 12
            out["list_straddles"] += ri <= 16 < ri + ng
            out["list_gt32"] += ri + ng > 32
            for i in np.flatnonzero(now):
                live.add((int(i) >> 8, int(i) & 3))
            for i in np.flatnonzero(gone):
                zero.add((int(i) >> 8, int(i) & 3))
            for x, y, p in idle_ranged:
                d2 = [(ex - x) ** 2 + (ey - y) ** 2 for (ex, ey), (_t, q) in at.items() if q == 1 - p]
                inside, outside = any(v <= RANGE * RANGE for v in d2), RANGE * RANGE + 1 in d2
                assert inside == bool(m[2 * g + p, y, x, 1 + ATTACK]), "the attack bit of a Ranged unit"
                out["ranged_left"] += x < RANGE and inside and outside
                out["ranged_top"] += y < RANGE and inside and outside
            out["ranged_none_after_some"] += step >= 2 and not idle_ranged and prev["ranged"][g] > 0
            if step >= 2 and not done[2 * g]:
                for p in range(2):
                    was, has = prev["prod"][g][p], prod[p]
                    if was is not None and has is not None and was != has:
                        paid = st.res[p] >= COST[WORKER]
                        assert paid == has, "the produce bit follows the player's resources"
                        out["afford_up" if has else "afford_down"] += 1
            if done[2 * g]:
                kind = "gameover" if rew[2 * g] != 0 else "timeout"
                out[f"{kind}_end{ends[step]}" if ends[step] <= 1 else f"{kind}_inside"] += 1
                out["reset_list_long"] += ng >= 12
        prev = cur
    ref.close()
    out["live"], out["zero"] = sorted(live), sorted(zero)
    return out
