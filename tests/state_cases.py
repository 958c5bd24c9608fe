"""Mid-game states for every map size of the reference traces, as GameState.toJSON text that both
the oracle and the HIP handle can take in (set_state_json): the states the recorded games pass
through, and crowded copies of them that hold every unit type, both owners and more than 64 units.
tests/test_gpu_every_shape.py steps the kernels from them against the oracle on all 17 map sizes;
tests/test_state_cases_cpu.py keeps the case list honest on the oracle alone.  Test infrastructure
only (a plain helper module, no fixtures of its own)."""
import ctypes
import functools
import gzip
import json
import os

import numpy as np

from tests import dumps, oracle_py
from tests.defs import COST, HP, NAMES, SEED  # noqa: F401  (SEED: re-exported)
from tests.dumps import live_units
from tests.trace_fixtures import GROUPS, ROOT, SIZES, TR  # noqa: F401  (SIZES: re-exported)

GAME_SEED = 3
TYPE_NAMES = [NAMES[t] for t in sorted(NAMES)]
MAX_HP = [HP[t] for t in sorted(HP)]
RESOURCE, WORKER = TYPE_NAMES.index("Resource"), TYPE_NAMES.index("Worker")


def dump_to_json(template_json, dump, type_names=TYPE_NAMES):
    """A canonical state dump (mrts_get_state's format: time, 2, res0, res1, nu, nu x (type, player, x, y,
    hp, res), na, na x (unit, type, parameter, x, y, unit type, time)) as GameState.toJSON text.  Terrain
    and size come from template_json, the state_json of a freshly reset game on the same map; unit IDs
    are list positions.  Only ATTACK_LOCATION (type 5) carries x / y (UnitAction.toJSON)."""
    time, res, units, assign = dumps.parse(dump)
    out = json.loads(template_json)
    out["time"] = time
    out["pgs"]["players"] = [{"ID": 0, "resources": res[0]}, {"ID": 1, "resources": res[1]}]
    out["pgs"]["units"] = [{"type": type_names[t], "ID": i, "player": p, "x": x, "y": y, "resources": r, "hitpoints": hp}
                           for i, (t, p, x, y, hp, r) in enumerate(units.tolist())]
    acts = []
    for unit, t, par, x, y, ut, when in assign.tolist():
        a = {"type": t}
        if t == 5:
            a["x"], a["y"] = x, y
        else:
            a["parameter"] = par
            if ut >= 0:
                a["unitType"] = type_names[ut]
        acts.append({"ID": unit, "time": when, "action": a})
    out["actions"] = acts
    return json.dumps(out, separators=(",", ":"))


@functools.lru_cache(maxsize=None)
def templates(size):
    """map path -> state_json of a freshly reset game, for every trace map of this size."""
    maps = sorted({e["map"] for e in GROUPS[size]})
    ref = oracle_py.OracleVecClient(2 * len(maps), 0, 2000, [m for m in maps for _ in range(2)])
    ref.reset()
    out = {m: ref.state_json(2 * i) for i, m in enumerate(maps)}
    ref.close()
    return out


@functools.lru_cache(maxsize=None)
def trace_states(size):
    """For every trace of this size (tests/golden/traces/index.json): the oracle's dumps at entries n//4,
    n//2, 3n//4 and n-1 of its replay -> [(map, fixture, entry, dump)]."""
    out = []
    for e in GROUPS[size]:
        text = gzip.open(os.path.join(TR, e["fixture"]), "rt").read()
        dumps, _ = oracle_py.trace_dumps(os.path.join(ROOT, e["map"]), text)
        n = len(dumps)
        for k in sorted({n // 4, n // 2, 3 * n // 4, n - 1}):
            out.append((e["map"], e["fixture"], k, dumps[k]))
    return out


def last_open_row(terrain, W, H):
    """The last row that holds a cell without wall.  The BroodWar maps (every map above 64x64 cells) close
    row H-1 with wall from end to end, so no unit can ever stand in it; there this is H-2."""
    return max(y for y in range(H) if "0" in terrain[y * W:(y + 1) * W])


def _windows(terrain, W, H, side=6):
    """About side x side cells at the four corners, at the centre and at the middle of the right edge; and
    one whose bottom row is the last open row, around that row's open cell nearest to the middle column
    (on a map whose last row is wall the corner windows may reach no open cell of the row above it)."""
    sw, sh = min(side, W), min(side, H)
    yb = last_open_row(terrain, W, H)
    xb = min((x for x in range(W) if terrain[yb * W + x] == "0"), key=lambda x: abs(x - W // 2))
    return [(0, 0, sw, sh), (W - sw, 0, sw, sh), (0, H - sh, sw, sh), (W - sw, H - sh, sw, sh),
            ((W - sw) // 2, (H - sh) // 2, sw, sh), (W - sw, (H - sh) // 2, sw, sh),
            (min(max(xb - sw // 2, 0), W - sw), max(yb + 1 - sh, 0), sw, sh)]


def crowd(state_json, seed, per_window=None):
    """state_json with units appended from a seeded generator: each a random type of all seven, a random
    owner (none for a Resource), hit points in 1..max, resources 1..29 for a Resource and 0/1 carried by a
    Worker; each player's resources become a random value in 0..14 on top of what the productions it has
    under way will cost (UnitAction.execute pays at completion; a player who cannot pay makes Java print
    "Illegal action attempted", the kernels' MRTS_ERR_NEG_RESOURCES).  The units go on free cells (no wall,
    no unit) of the windows of _windows, per_window each (default 14 on maps of >= 144 cells, else
    3), and never on a cell 4-adjacent to a unit the state already holds: a pending PRODUCE or MOVE of
    that unit would land on the new one (PhysicalGameState.addUnit throws "added two units in
    position")."""
    rng = np.random.default_rng(seed)
    d = json.loads(state_json)
    pgs = d["pgs"]
    W, H = pgs["width"], pgs["height"]
    if per_window is None:
        per_window = 14 if W * H >= 144 else 3
    taken = np.array([c != "0" for c in pgs["terrain"]], bool).reshape(H, W)
    for u in pgs["units"]:
        for dx, dy in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1)):
            x, y = u["x"] + dx, u["y"] + dy
            if 0 <= x < W and 0 <= y < H:
                taken[y, x] = True
    for x0, y0, w, h in _windows(pgs["terrain"], W, H):
        free = [(x, y) for y in range(y0, y0 + h) for x in range(x0, x0 + w) if not taken[y, x]]
        for i in rng.permutation(len(free))[:per_window]:
            x, y = free[i]
            t = int(rng.integers(0, 7))
            hp = int(rng.integers(1, MAX_HP[t] + 1))
            res = int(rng.integers(1, 30)) if t == RESOURCE else int(rng.integers(0, 2)) if t == WORKER else 0
            player = -1 if t == RESOURCE else int(rng.integers(0, 2))
            pgs["units"].append({"type": TYPE_NAMES[t], "ID": len(pgs["units"]), "player": player, "x": x, "y": y,
                                 "resources": res, "hitpoints": hp})
            taken[y, x] = True
    owner = {u["ID"]: u["player"] for u in pgs["units"]}
    for p in pgs["players"]:
        due = sum(COST[TYPE_NAMES.index(a["action"]["unitType"])] for a in d["actions"] if a["action"]["type"] == 4 and owner[a["ID"]] == p["ID"])
        p["resources"] = due + int(rng.integers(0, 15))
    return json.dumps(d, separators=(",", ":"))


def state_probe(name, size, max_units, text, cap=1 << 18, utt_version=1, crs=1, utt_json=None):
    """The product's own state converters without a handle or a GPU (mrts_hostdata.cpp, beside jsonToBlock; not in
    include/mrts.h): name = "mrts_internal_state_probe" (text -> a zeroed state block -> text) or
    "mrts_internal_dump_probe" (... -> the canonical dump's words), for a handle of this size as mrts_create sizes it
    -> (return value, the int32 buffer written: cap words, the refusal's text)."""
    from microrts_amd import _lib

    f = getattr(_lib.load(), name)
    I, C, P = ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p
    f.argtypes, f.restype = [I, I, I, I, I, I, C, C, P, I, C, I], I
    H, W = size
    mu = min(max_units, H * W) if max_units else H * W
    out = np.zeros(cap, np.int32)
    err = ctypes.create_string_buffer(256)
    n = f(H, W, mu + max(64, mu // 4), mu, utt_version, crs, utt_json, text.encode(), out.ctypes.data_as(ctypes.c_void_p),
          cap * (4 if name == "mrts_internal_state_probe" else 1), err, 256)
    return n, out, err.value.decode()


def budget(size):
    """(games, steps, max_steps, max_units) of a size's case.  max_steps lies below the stepped horizon:
    envSteps restarts at 0 on injection, so every game times out and resets inside a step."""
    H, W = size
    big = H * W > 64 * 64
    return (8, 20, 14, 1024) if big else (24, 30, 22, 0)


@functools.lru_cache(maxsize=None)
def case(size):
    """The games of one map size: every other one a state of a recorded game as it is, the others crowded
    copies (crowd, seeded by the game's index) -> dict(size, maps [one per self-play slot], states [one JSON
    per game], crowded [bool per game], trace_units [units per game before crowding], steps, max_steps,
    max_units, edge_row [the last row open in any of the maps])."""
    n_games, steps, max_steps, max_units = budget(size)
    st = trace_states(size)
    tm = templates(size)
    pick = [st[(i * len(st)) // n_games] for i in range(n_games)] if len(st) >= n_games else \
        [st[i % len(st)] for i in range(n_games)]
    maps, states, crowded, trace_units = [], [], [], []
    for g, (mp, _fx, _k, dump) in enumerate(pick):
        j = dump_to_json(tm[mp], dump)
        crowded.append(g % 2 == 1)
        trace_units.append(dumps.n_units(dump))
        states.append(crowd(j, 1000 * size[0] + 10 * size[1] + g) if crowded[-1] else j)
        maps += [mp, mp]
    edge_row = max(last_open_row(json.loads(tm[mp])["pgs"]["terrain"], size[1], size[0]) for mp in set(maps))
    return dict(size=size, maps=maps, states=states, crowded=crowded, steps=steps, max_steps=max_steps, max_units=max_units,
                edge_row=edge_row, trace_units=trace_units)


BOT_SIZES = [(8, 9), (12, 14), (96, 128)]  # (H, W) of the 9x8, 14x12 and 128x96 maps


def bot_case(size):
    """The agent-vs-bot form of case(size): one env per game (at most 8), players alternating 0 / 1."""
    c = case(size)
    n = min(8, len(c["states"]))
    return dict(c, maps=c["maps"][0:2 * n:2], states=c["states"][:n], crowded=c["crowded"][:n], trace_units=c["trace_units"][:n],
                players=[0, 1] * (n // 2))


def java_rows(acts, reverse):
    """Grid actions [slots][HW][7] as Java rows [slots][HW][8] = [pos, 7 components], ascending or reversed."""
    S, HW, _ = acts.shape
    rows = np.concatenate([np.broadcast_to(np.arange(HW, dtype=np.int32)[None, :, None], (S, HW, 1)), acts], axis=2)
    return np.ascontiguousarray(rows[:, ::-1] if reverse else rows, np.int32)


def oracle_run(c, partial_obs=False):
    """The GPU test's self-play rollout of case c on the oracle alone (its own Philox rows from its own
    masks, which the GPU test proves equal to the kernels') -> what the run reaches."""
    n = len(c["states"])
    S = 2 * n
    ref = oracle_py.OracleVecClient(S, 0, c["max_steps"], c["maps"], partial_obs=partial_obs, seed=GAME_SEED)
    ref.reset()
    for g, j in enumerate(c["states"]):
        ref.set_state_json(2 * g, j)
    out = dict(types=set(), owners=set(), most_units=0, last_col=0, last_row=0, attack_bits=0, deaths=0, resets=0, errors=0)
    for g in range(n):
        u = live_units(ref.dump(2 * g))
        out["types"] |= set(u[:, 0].tolist())
        out["owners"] |= set(u[:, 1].tolist())
        out["most_units"] = max(out["most_units"], len(u))
    for step in range(c["steps"]):
        m = ref.get_masks(0)
        out["last_col"] += int(m[:, :, -1, 0].sum())
        out["last_row"] += int(m[:, c["edge_row"], :, 0].sum())
        out["attack_bits"] += int(m[..., 30:].sum())
        owned = [int((live_units(ref.dump(2 * g))[:, 1] >= 0).sum()) for g in range(n)]
        _, _, done = ref.step(np.stack([oracle_py.policy(m[s], SEED, s, step, 0) for s in range(S)]))
        for g in range(n):
            out["errors"] += int(ref.L.oref_errors(ref.h, 2 * g))  # Java's prints ("Illegal action attempted", ...)
            if done[2 * g]:
                out["resets"] += 1
            elif int((live_units(ref.dump(2 * g))[:, 1] >= 0).sum()) < owned[g]:
                out["deaths"] += 1  # fewer owned units after a step without a reset: one was killed
    ref.close()
    return out
