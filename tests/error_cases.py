"""States that end in one of the step kernels' error branches (the per-game MRTS_ERR_* bits), as GameState.toJSON
text that both the oracle and the HIP handle take in: an action under way that cannot complete as issued.
tests/test_gpu_error_flags.py steps the kernels from them; tests/test_error_cases_cpu.py shows on the oracle alone
that each scenario happens.  Test infrastructure only (a plain helper module, no fixtures of its own).

Every builder returns (faulty_json, twin_json, fires_at): the doomed action completes in the fires_at-th step after
the injection (GameState.cycle: issue time + ETA <= time, so its `time` field is state time + fires_at - ETA), and
the twin is the same state with each doomed action replaced by a NONE issued at the same time and completing in the
same cycle.  The twin is what the kernels' branch leaves of MRTS_ERR_ADDUNIT and MRTS_ERR_CAPACITY (the assignment
leaves the map, nothing is produced, nothing is paid), where Java throws or has no counterpart; for
MRTS_ERR_NEG_RESOURCES the oracle itself goes on (Java prints), so the faulty state on the oracle is the reference.

No state here leaves the map: every MOVE / PRODUCE target is a cell of it (the builders assert so, and jsonToBlock
refuses any other), and the capacity case ends at the `nu >= CAP` guard of UnitAction.execute's PRODUCE branch."""
import json

import numpy as np

from tests import dumps, oracle_py
from tests import state_cases as SC
from tests.defs import BASE, COST, DX, DY, HP, MOVE, NAMES, NONE, PRODUCE, RESOURCE, WORKER

T0 = 100                    # the injected states' time: later than any ETA, so every issue time is positive
WORKER_PRODUCE_TIME = 50    # UnitTypeTable VERSION_ORIGINAL (UnitTypeTable.java:150-168): the ETA of PRODUCE Worker
WORKER_MOVE_TIME = 10       # ... and of a Worker's MOVE
BUSY = 1000                 # the duration of a NONE that keeps a unit out of the way
GAMES, FAULTY = 8, (2, 5)   # a handle's games, and the ones that get the faulty state
E_CAPACITY, E_ADDUNIT, E_PRODUCE_TYPE, E_OLDER_CONFLICT, E_NEG_RESOURCES, E_MOVE_COLLISION = (1 << b for b in range(6))
MAPS = {(8, 8): "maps/8x8/basesWorkers8x8.xml", (10, 10): "maps/10x10/basesWorkers10x10.xml",
        (12, 12): "maps/12x12/basesWorkers12x12.xml", (16, 16): "maps/16x16/basesWorkers16x16.xml",
        (32, 32): "maps/basesWorkers32x32A.xml"}
CAPACITY_SIZE, CAPACITY_UNITS = (16, 16), 68


def _fresh(size):
    """The freshly reset game on the size's map at time T0, unit IDs = list positions (as the build writes them, and
    as SC.crowd continues them), no actions."""
    d = json.loads(SC.templates(size)[MAPS[size]])
    d["time"] = T0
    for i, u in enumerate(d["pgs"]["units"]):
        u["ID"] = i
    d["actions"] = []
    return d


def _text(d):
    return json.dumps(d, separators=(",", ":"))


def _unit(d, type_name, player):
    return next(u for u in d["pgs"]["units"] if u["type"] == type_name and u["player"] == player)


def _free_neighbour(d, u):
    """(direction, x, y) of the first 4-neighbour of unit u that is a cell of the map without wall or unit"""
    pgs = d["pgs"]
    W, H = pgs["width"], pgs["height"]
    taken = {(v["x"], v["y"]) for v in pgs["units"]}
    for k in (1, 2, 3, 0):  # right, down, left, up
        x, y = u["x"] + DX[k], u["y"] + DY[k]
        if 0 <= x < W and 0 <= y < H and pgs["terrain"][y * W + x] == "0" and (x, y) not in taken:
            return k, x, y
    raise AssertionError("no free cell next to the unit")


def _add(d, t, player, x, y):
    d["pgs"]["units"].append({"type": NAMES[t], "ID": len(d["pgs"]["units"]), "player": player, "x": x, "y": y,
                              "resources": 0, "hitpoints": HP[t]})


def _assign(d, u, action, fires_at, eta):
    assert fires_at >= 1
    d["actions"].append({"ID": u["ID"], "time": d["time"] + fires_at - eta, "action": action})


def _produce_worker(direction):
    return {"type": PRODUCE, "parameter": direction, "unitType": NAMES[WORKER]}


def twin_of(faulty_json, doomed):
    """faulty_json with the action of every unit ID in `doomed` replaced by the NONE that completes in its cycle"""
    d = json.loads(faulty_json)
    eta = {PRODUCE: WORKER_PRODUCE_TIME, MOVE: WORKER_MOVE_TIME}
    n = 0
    for a in d["actions"]:
        if a["ID"] in doomed:
            a["action"] = {"type": NONE, "parameter": eta[a["action"]["type"]]}
            n += 1
    assert n == len(doomed)
    return _text(d)


def _targets_on_map(text):
    d = json.loads(text)
    pgs = d["pgs"]
    at = {u["ID"]: (u["x"], u["y"]) for u in pgs["units"]}
    for a in d["actions"]:
        if a["action"]["type"] in (MOVE, PRODUCE):
            k = a["action"]["parameter"]
            x, y = at[a["ID"]][0] + DX[k], at[a["ID"]][1] + DY[k]
            assert 0 <= x < pgs["width"] and 0 <= y < pgs["height"], f"unit {a['ID']}'s target ({x}, {y}) is off the map"
    return text


def _finish(d, doomed, fires_at, crowd_seed, resources=None):
    text = _text(d)
    if crowd_seed is not None:  # past 64 units, never next to a unit
        text = SC.crowd(text, crowd_seed, per_window=CROWD_PER_WINDOW)
        if resources is not None:  # (crowd gives each player what its productions cost, and more)
            e = json.loads(text)
            for p, r in zip(e["pgs"]["players"], resources):
                p["resources"] = r
            text = _text(e)
        assert len(json.loads(text)["pgs"]["units"]) > 64, "the crowded variant is for the paths past one wave of units"
    else:
        assert len(d["pgs"]["units"]) <= 64
    return _targets_on_map(text), _targets_on_map(twin_of(text, doomed)), fires_at


def neg_resources(size, fires_at=10, crowd_seed=None):
    """Player 0's Base holds PRODUCE Worker toward a free cell, and player 0 owns nothing: UnitAction.execute skips
    the production (Java prints "Illegal action attempted", UnitAction.java:457-461) -> MRTS_ERR_NEG_RESOURCES."""
    d = _fresh(size)
    base = _unit(d, "Base", 0)
    k, _, _ = _free_neighbour(d, base)
    _assign(d, base, _produce_worker(k), fires_at, WORKER_PRODUCE_TIME)
    for p, r in zip(d["pgs"]["players"], (0, 5)):
        p["resources"] = r
    assert d["pgs"]["players"][0]["resources"] < COST[WORKER]
    return _finish(d, {base["ID"]}, fires_at, crowd_seed, resources=(0, 5))


def addunit(size, fires_at=1, crowd_seed=None):
    """The same PRODUCE, paid for, with a Worker of player 1 standing on the target cell: PhysicalGameState.addUnit
    throws "added two units in position" (PhysicalGameState.java:190-195) -> MRTS_ERR_ADDUNIT."""
    d = _fresh(size)
    base = _unit(d, "Base", 0)
    k, x, y = _free_neighbour(d, base)
    _add(d, WORKER, 1, x, y)
    _assign(d, base, _produce_worker(k), fires_at, WORKER_PRODUCE_TIME)
    for p in d["pgs"]["players"]:
        p["resources"] = 5
    return _finish(d, {base["ID"]}, fires_at, crowd_seed)


def collision(size, fires_at=1):
    """Player 0's Worker holds a MOVE onto a cell where a Worker of player 1 stands -> MRTS_ERR_MOVE_COLLISION.  Java
    moves it there without a word; two units then share a cell, and what follows is outside every contract."""
    d = _fresh(size)
    w = _unit(d, "Worker", 0)
    k, x, y = _free_neighbour(d, w)
    _add(d, WORKER, 1, x, y)
    _assign(d, w, {"type": MOVE, "parameter": k}, fires_at, WORKER_MOVE_TIME)
    return _finish(d, {w["ID"]}, fires_at, None)


def capacity(producers, fires_at=1):
    """A 16x16 game for a handle of max_units = CAPACITY_UNITS = 68 (so CAP = 68 + max(64, 68 / 4) = 132 unit
    slots): exactly 68 units, the first `producers` of them Bases of player 0 on the even columns of rows 0 .. 8,
    each holding PRODUCE Worker to the free cell on its right, all issued at one time in list order and all paid
    for (100 resources); the rest belong to player 1 or to nobody (with no unit of player 1 the game would be over),
    and player 1's hold a long NONE, so the producers' are the only assignments ready in the firing cycle.
    64 producers: every birth lands and nu reaches CAP exactly.  66: the first 64 land in list order, the last two
    meet nu >= CAP -> MRTS_ERR_CAPACITY (no Java equivalent); their NONE twins are the reference.  More than 64
    ready assignments is also the only way into the repeated minimum search of the kernels' cycle()."""
    assert 64 <= producers <= CAPACITY_UNITS - 2
    d = _fresh(CAPACITY_SIZE)
    assert len(d["pgs"]["units"]) <= CAPACITY_UNITS, "a map holds more units than max_units"
    assert "1" not in d["pgs"]["terrain"]
    d["pgs"]["units"] = []
    cells = [(x, y) for y in range(9) for x in range(0, 16, 2)][:producers]
    for x, y in cells:
        _add(d, BASE, 0, x, y)
    rest = [(BASE, 1, 13, 13), (WORKER, 1, 14, 14), (RESOURCE, -1, 15, 15), (RESOURCE, -1, 15, 14)]
    for t, p, x, y in rest[:CAPACITY_UNITS - producers]:
        _add(d, t, p, x, y)
        if t == RESOURCE:
            d["pgs"]["units"][-1]["resources"] = 20
    assert len(d["pgs"]["units"]) == CAPACITY_UNITS
    for u in d["pgs"]["units"][:producers]:
        _assign(d, u, _produce_worker(1), fires_at, WORKER_PRODUCE_TIME)
    for u in d["pgs"]["units"][producers:]:  # an idle owned unit would be given a NONE that is ready at once
        if u["player"] >= 0:
            d["actions"].append({"ID": u["ID"], "time": T0, "action": {"type": NONE, "parameter": BUSY}})
    for p, r in zip(d["pgs"]["players"], (100, 5)):
        p["resources"] = r
    text = _targets_on_map(_text(d))
    refused = set(range(64, producers))
    return text, _targets_on_map(twin_of(text, refused)), fires_at


def games(size, faulty_json, max_units=None):
    """The GAMES states of one handle: faulty_json for the games of FAULTY, and for the others states that the
    recorded games on the same map pass through (SC.trace_states), as they are: the controls."""
    mp = MAPS[size]
    plain = [s[3] for s in SC.trace_states(size) if s[0] == mp]
    if max_units is not None:
        plain = [p for p in plain if dumps.n_units(p) <= max_units]
    assert len(plain) >= GAMES - len(FAULTY)
    it = iter(plain)
    return [faulty_json if g in FAULTY else SC.dump_to_json(SC.templates(size)[mp], next(it)) for g in range(GAMES)]


def oracle(size, states, max_steps=2000, bots=False, partial_obs=False):
    """The oracle's handle of these games (two self-play slots per game, or one agent-vs-RandomBiasedAI env per game),
    reset, with the states injected."""
    n = len(states)
    mp = MAPS[size]
    if bots:
        ref = oracle_py.OracleVecClient(0, n, max_steps, [mp] * n, partial_obs=partial_obs, seed=SC.GAME_SEED,
                                        bot_kinds=[oracle_py.BOT_RANDOM_BIASED] * n)
    else:
        ref = oracle_py.OracleVecClient(2 * n, 0, max_steps, [mp] * (2 * n), partial_obs=partial_obs, seed=SC.GAME_SEED)
    ref.reset()
    for g, j in enumerate(states):
        ref.set_state_json((1 if bots else 2) * g, j)
    return ref


def masked_rows(ref, step):
    """Every slot's masked-random rows of this step (the policy kernel's, bit for bit)"""
    m = ref.get_masks(0)
    return np.stack([oracle_py.policy(m[s], SC.SEED, s, step, 0) for s in range(ref.S)])


def zero_rows(ref):
    return np.zeros((ref.S, ref.H * ref.W, 7), np.int32)


def errors(ref):
    """The oracle's count of Java's prints per slot"""
    return np.array([ref.L.oref_errors(ref.h, s) for s in range(ref.S)])


def counts(dump):
    """(units, units with an owner) of a dump.  A unit holds at most one assignment, so the second bounds the ready
    assignments of any cycle: with more than 64 units and at most 64 owned ones the kernels' cycle() gathers its
    LDS ready list; with at most 64 units it runs one unit per lane."""
    u = dumps.live_units(dump)
    return len(u), int((u[:, 1] >= 0).sum())


# (scenario, size, crowd seed or None) of the self-play cases both test files run.  A crowd of CROWD_PER_WINDOW units
# per window takes the 16x16, 12x12 and 32x32 games past 64 units while the owned ones stay at 64 or fewer.
CROWD_PER_WINDOW = 9
NEG_CASES = [((10, 10), None), ((8, 8), None), ((16, 16), None), ((16, 16), 11), ((32, 32), 12)]
ADDUNIT_CASES = [((12, 12), None), ((12, 12), 13), ((16, 16), None), ((16, 16), 14)]
COLLISION_SIZES = [(10, 10), (16, 16)]
PO_MAX_UNITS = 256  # the 32x32 partially observable instance's


def case_id(c):
    (h, w), seed = c
    return f"{w}x{h}{' crowded' if seed is not None else ''}"


# the older-conflict branch of GameState.issue (GameState.java:298-317), in tests/trace_fixtures.py's text format on
# maps/melee4x4light2.xml (four Lights: 32 at (0,0) and 33 at (0,1) of player 0, 34 at (3,2) and 35 at (3,3) of
# player 1; a Light's MOVE takes 8 cycles).  Light 32 moves right to (1,0), then down toward (1,1); while that move
# is under way Light 33 is told to move right to (1,1) too: the cell is reserved by an assignment issued earlier
# (time 8, not 10), so Java prints "Inconsistent actions were executed!" and gives Light 33 a NONE of parameter -1,
# which the next cycle ends: a second entry at time 10, without actions, is where a dump shows it.
OLDER_MAP = "maps/melee4x4light2.xml"
_LIGHTS = "U 4 33 0 0 1 0 4\nU 4 34 1 3 2 0 4\nU 4 35 1 3 3 0 4\n"
OLDER_CONFLICT_TRACE = (
    "TRACE 5\n"
    "E 0\nP 0 0\nN 4\nU 4 32 0 0 0 0 4\n" + _LIGHTS + "A 1\na 32 1 1 0 0 -1\n"
    "E 8\nP 0 0\nN 4\nU 4 32 0 1 0 0 4\n" + _LIGHTS + "A 1\na 32 1 2 0 0 -1\n"
    "E 10\nP 0 0\nN 4\nU 4 32 0 1 0 0 4\n" + _LIGHTS + "A 1\na 33 1 1 0 0 -1\n"
    "E 10\nP 0 0\nN 4\nU 4 32 0 1 0 0 4\n" + _LIGHTS + "A 0\n"
    "E 20\nP 0 0\nN 4\nU 4 32 0 1 1 0 4\n" + _LIGHTS + "A 0\n")
OLDER_ENTRY = 2  # the entry whose action is refused
