"""Scenario helpers for the combat-unit tests: maps that put Light, Heavy and Ranged units, attacks of
range > 1 and games that end by elimination in front of the output kernels within a few hundred steps
(the random-policy rollouts from basesWorkers* starts never reach them: DESIGN.md, "What the random
rollouts never reach").  Built on tests.defs.write_map; every map is written by the test that
uses it.  Also the census the adequacy tests assert on (oracle only, no GPU)."""
import numpy as np

from tests import oracle_py
from tests.defs import HEAVY, LIGHT, RANGED, RESOURCE, SEED, WORKER, write_map

GAME_SEED = 3  # tests.gpu_checks.rollout's default game seed

MELEE16 = "maps/16x16/melee16x16Mixed12.xml"
MELEE8 = "maps/8x8/melee8x8Mixed6.xml"
MELEE14X12 = "maps/melee14x12Mixed18.xml"
MELEE12 = "maps/12x12/melee12x12Mixed12.xml"
BARRACKS16 = "maps/16x16/TwoBasesBarracks16x16.xml"

ALL_RFS = ["WinLossRewardFunction", "ResourceGatherRewardFunction", "ProduceWorkerRewardFunction",
           "ProduceBuildingRewardFunction", "AttackRewardFunction", "ProduceCombatUnitRewardFunction",
           "CloserToEnemyBaseRewardFunction", "CloserToEnemyUnitRewardFunction"]


def arena(path, W, H, variant):
    """A walled 4x3 enclosure in a map corner, no resources: player a's Heavy and Ranged against player
    b's Worker and Light, four cells apart, so the random policy ends the game by elimination within a
    few hundred steps.  Variant bit 1 picks the corner (clear: top left, set: bottom right), bit 0
    swaps the players."""
    if variant & 2:
        ox, oy = W - 4, H - 3
        walls = [(W - 5, y) for y in range(H - 4, H)] + [(x, H - 4) for x in range(W - 4, W)]
    else:
        ox, oy = 0, 0
        walls = [(4, y) for y in range(4)] + [(x, 3) for x in range(4)]
    a, b = (1, 0) if variant & 1 else (0, 1)
    units = [(HEAVY, a, ox, oy), (RANGED, a, ox, oy + 2), (WORKER, b, ox + 3, oy + 1), (LIGHT, b, ox + 3, oy + 2)]
    return write_map(path, W, H, units, walls=walls, res=(0, 0))


def arena_maps(tmp_path, W, H, n_slots, tag="arena"):
    """One map path per slot: game g (slots 2g, 2g + 1) plays variant g % 4."""
    paths = [arena(tmp_path / f"{tag}{W}x{H}_v{v}.xml", W, H, v) for v in range(4)]
    return [paths[(s // 2) % 4] for s in range(n_slots)]


def mixed_maps(tmp_path, n_slots):
    """Arena-16x16 games and melee16x16Mixed12 games alternating, both slots of a game on one map."""
    ar = arena_maps(tmp_path, 16, 16, n_slots)
    return [ar[s] if (s // 2) % 2 == 0 else MELEE16 for s in range(n_slots)]


def in_range(dx, dy, r=3):
    """Attack range r (Ranged's 3 in the built-in tables) in the rule of Unit.getUnitActions (Unit.java:424-431)."""
    return dx * dx + dy * dy <= r * r


def window_enemy(dx, dy, flip):
    """The fixed pattern of ranged_window: which cells of the 9x9 block hold an enemy."""
    return bool(((dx + 4) * 3 + (dy + 4) * 5 + ((dx + 4) * (dy + 4)) // 3) & 1) != bool(flip)


def ranged_window(path, W, H, cx, cy, flip, r=3):
    """A Ranged unit of player 0 (attack range r) at (cx, cy); every other in-map cell of the block of
    2r + 3 cells a side around it (9x9 for r = 3) holds an enemy Worker, an own Light or a Resource unit.
    `flip` exchanges the enemy cells and the non-enemy cells, so over the two layouts each of the offsets
    in range (28 for r = 3, 12 for r = 2) is set once and clear once.
    -> (path, layout): layout[(x, y)] = (type, player)."""
    layout = {(cx, cy): (RANGED, 0)}
    for dy in range(-r - 1, r + 2):
        for dx in range(-r - 1, r + 2):
            x, y = cx + dx, cy + dy
            if (dx, dy) == (0, 0) or not (0 <= x < W and 0 <= y < H):
                continue
            if window_enemy(dx, dy, flip):
                layout[(x, y)] = (WORKER, 1)
            elif (dx - dy) % 3 == 0:
                layout[(x, y)] = (LIGHT, 0)
            else:
                layout[(x, y)] = (RESOURCE, -1)
    cells = sorted(layout.items(), key=lambda c: (c[0][1], c[0][0]))  # unit list in row-major order
    units = [(t, p, x, y) + ((7,) if t == RESOURCE else ()) for (x, y), (t, p) in cells]
    return write_map(path, W, H, units, res=(0, 0)), layout


def skirmish32(path):
    """A 32x32 skirmish for the partially observable records exchange: Light, Heavy and Ranged units
    (and a Worker) of both players a few cells apart in the middle of the map, so radius-2 and
    radius-3 sight disks overlap enemy units from the first step."""
    units = []
    for p, x0, step in ((0, 14, 1), (1, 17, -1)):
        for i, t in enumerate((LIGHT, HEAVY, RANGED, WORKER, LIGHT, HEAVY, RANGED)):
            units.append((t, p, x0 + step * (i % 2), 10 + 2 * i))
    units += [(RESOURCE, -1, 15, 8, 10), (RESOURCE, -1, 16, 24, 10)]
    return write_map(path, 32, 32, units, res=(0, 0))


def _sc(id, kind, maps, po=False, utt=1, crs=1, max_units=0, n_bot=0, n_slots=16, steps=300, players=None):
    return dict(id=id, kind=kind, maps=maps, po=po, utt=utt, crs=crs, max_units=max_units, n_bot=n_bot, n_slots=n_slots,
                steps=steps, players=players)


def _fixed(mp):
    return lambda tmp_path, n: [mp] * n


def _arena(W, H):
    return lambda tmp_path, n: arena_maps(tmp_path, W, H, n)


# Every rollout scenario of tests/test_gpu_combat.py; tests/test_combat_scenarios.py asserts on the oracle
# alone that each still reaches what it is there for.  maps(tmp_path, n_slots) -> one path per slot.
ROLLOUTS = [
    _sc("melee16", "melee", _fixed(MELEE16)),
    _sc("melee16-po", "melee", _fixed(MELEE16), po=True),
    _sc("melee8-utt3-crs1", "melee", _fixed(MELEE8), utt=3, crs=1),
    _sc("melee8-utt3-crs2", "melee", _fixed(MELEE8), utt=3, crs=2),
    _sc("melee14x12", "melee", _fixed(MELEE14X12)),
    _sc("melee14x12-po", "melee", _fixed(MELEE14X12), po=True),
    _sc("melee12-utt2", "melee", _fixed(MELEE12), utt=2),
    _sc("barracks16", "barracks", _fixed(BARRACKS16)),
    _sc("arena16", "arena", _arena(16, 16)),
    _sc("arena16-utt3", "arena", _arena(16, 16), utt=3),
    _sc("arena8", "arena", _arena(8, 8)),
    _sc("arena14x12", "arena", _arena(14, 12)),
    _sc("arena32-po", "arena", _arena(32, 32), po=True, max_units=256),
    _sc("melee8-bots", "melee", _fixed(MELEE8), n_bot=8, n_slots=8, players=[0, 1] * 4),
    _sc("melee8-bots-po", "melee", _fixed(MELEE8), n_bot=8, n_slots=8, players=[0, 1] * 4, po=True),
]

def census(maps, n_slots=16, steps=300, partial_obs=False, utt=1, crs=1, max_steps=2000, rfs=None, n_bot=0,
           players=None):
    """The suite's masked rollout on the oracle alone (game seed 3, policy seed SEED, masks of player 0):
    what the rollout reaches, counted over every step.  n_bot: that many of the slots are
    agent-vs-RandomBiasedAI games (then no self-play pairs)."""
    ref = oracle_py.OracleVecClient(n_slots - n_bot, n_bot, max_steps, maps, partial_obs=partial_obs, utt_version=utt, crs=crs,
                                    seed=GAME_SEED, bot_kinds=[oracle_py.BOT_RANDOM_BIASED] * n_bot if n_bot else None,
                                    rewards=[oracle_py.REWARD_IDS[r] for r in rfs] if rfs else None)
    obs, _, _ = ref.reset(players)
    out = {"types": np.zeros(8, np.int64), "attack_bits": 0, "attack_outer": 0, "produce_types": np.zeros(7, np.int64),
           "terminal": 0, "pairs": [], "attack_reward": 0, "enemy_combat_seen": 0}
    centre = np.zeros((7, 7), bool)
    centre[2:5, 2:5] = True
    for step in range(steps):
        m = ref.get_masks(0)
        out["types"] += np.bincount(obs[:, 3].ravel().clip(0, 7), minlength=8)
        out["enemy_combat_seen"] += int(((obs[:, 2] == 2) & (obs[:, 3] > WORKER + 1)).sum())
        att = m[..., 30:79].reshape(-1, 7, 7)
        out["attack_bits"] += int(att.sum())
        out["attack_outer"] += int(att[:, ~centre].sum())
        out["produce_types"] += m[..., 23:30].reshape(-1, 7).sum(axis=0, dtype=np.int64)
        acts = np.stack([oracle_py.policy(m[s], SEED, s, step, 0) for s in range(n_slots)])
        obs, rew, done = ref.step(acts, players)
        if rfs:
            out["attack_reward"] += int((rew[:, ALL_RFS.index("AttackRewardFunction")] != 0).sum())
            rew, done = rew[:, 0], done[:, 0]
        out["terminal"] += int(done.sum())
        for g in range(n_slots // 2):
            if done[2 * g] and rew[2 * g] != 0:
                out["pairs"].append((float(rew[2 * g]), float(rew[2 * g + 1])))
    ref.close()
    return out
