"""Unit-type tables whose mask layout differs from the built-in one (a plain helper module, no tests).

A table sets the width of every mask row and action row: K = 1 + 22 + ntypes + R * R with
R = 2 * maxAttackRange + 1 (JNIGridnetClient.java:125,138).  The built-in tables and the reference's fixture
all give K = 79 (7 types, R = 7); the tables here give the other window sizes and type counts that
mrts_create accepts.  Each is made by editing the product's own UnitTypeTable(...).toJSON(), as
tests/test_gpu_parity.py test_utt_from_json_eight_types does; no file of the reference is involved.

TABLES[id] = Table(id, version, crs, nt, R, K, far): the built-in table edited, the expected numbers
(written down here, pinned against the oracle and the product's parser by tests/test_table_cases_cpu.py) and the
names of the types with attackRange > 1."""
import collections
import functools
import json

import numpy as np

Table = collections.namedtuple("Table", "id version crs nt R K far")

TABLES = {
    "r5": Table("r5", 1, 1, 7, 5, 55, ("Ranged",)),
    "r3": Table("r3", 1, 1, 7, 3, 39, ()),
    "t5r3": Table("t5r3", 1, 1, 5, 3, 37, ()),
    "t8r5": Table("t8r5", 2, 3, 8, 5, 56, ("Ranged", "Tower")),
}
IDS = list(TABLES)

# the 8th type of test_utt_from_json_eight_types: absent members take UnitType.updateFromJSON's defaults
TOWER = {"ID": 7, "name": "Tower", "cost": 3, "hp": 6, "attackRange": 2, "minDamage": 1, "maxDamage": 3, "canAttack": True,
         "sightRadius": 4, "produces": [], "producedBy": ["Worker"]}
KEEP5 = ("Resource", "Base", "Barracks", "Worker", "Light")


@functools.lru_cache(maxsize=None)
def utt_json(id):
    """The JSON text of table `id`."""
    from microrts_amd.vec_client import UnitTypeTable

    c = TABLES[id]
    t = json.loads(UnitTypeTable(c.version, c.crs).toJSON())
    types = t["unitTypes"]
    by = {u["name"]: u for u in types}
    if id == "r5":
        by["Ranged"]["attackRange"] = 2
    elif id == "r3":
        by["Ranged"]["attackRange"] = 1
    elif id == "t5r3":
        types = [u for u in types if u["name"] in KEEP5]
        for i, u in enumerate(types):
            u["ID"] = i
            u["produces"] = [n for n in u["produces"] if n in KEEP5]
            u["producedBy"] = [n for n in u["producedBy"] if n in KEEP5]
        t["unitTypes"] = types
    elif id == "t8r5":
        by["Ranged"]["attackRange"] = 2
        by["Worker"]["produces"].append("Tower")
        types.append(dict(TOWER))
    return json.dumps(t)


def attack_range(id, name):
    """attackRange of type `name` in table `id`."""
    return next(u["attackRange"] for u in json.loads(utt_json(id))["unitTypes"] if u["name"] == name)


def atk_base(c):
    """The first attack slot of a mask row: 1 own-idle + 6 action types + 4 * 4 directions + nt produce types."""
    return 23 + c.nt


def atk_index(c, dx, dy):
    """The attack component of an action on the cell at offset (dx, dy): UnitAction.java:701-702 read backwards,
    (dy + maxAttackRange) * R + (dx + maxAttackRange)."""
    return (c.R // 2 + dy) * c.R + (c.R // 2 + dx)


def disk(c, r=None):
    """bool[R][R]: the offsets a unit of range r (default: the table's largest) can attack, dx^2 + dy^2 <= r^2
    without the unit's own cell (Unit.java:424-434), placed in the table's window."""
    ctr = c.R // 2
    r = ctr if r is None else r
    return np.array([[(dx, dy) != (0, 0) and dx * dx + dy * dy <= r * r for dx in range(-ctr, ctr + 1)]
                     for dy in range(-ctr, ctr + 1)])


class Reach:
    """What a rollout's masks reached, counted on the oracle's side: which attack slots of the window and which
    action-type bits were ever set."""

    def __init__(self, c):
        self.c = c
        self.window = np.zeros((c.R, c.R), bool)
        self.types = np.zeros(6, bool)

    def add(self, masks):
        m = masks.reshape(-1, self.c.K)
        self.window |= m[:, atk_base(self.c):].any(axis=0).reshape(self.c.R, self.c.R)
        self.types |= m[:, 1:7].any(axis=0)


MELEE8, BASES8, NOWHERE = "maps/8x8/melee8x8Mixed6.xml", "maps/8x8/basesWorkers8x8.xml", "maps/NoWhereToRun9x8.xml"
N_SP, N_BOT, GAME_SEED = 8, 2, 3  # every step-parity rollout: 8 self-play slots + 2 RandomBiasedAI envs, game seed 3

Step = collections.namedtuple("Step", "id table map policy steps po reach types")
# reach: what the oracle's masks of the rollout must have shown (check_reach):
#   "disk"  every in-disk attack slot of the table's window, and the action-type bits of `types`;
#   "some"  the ATTACK bit, and for a table with a far type an attack slot more than one cell away (the 16x16
#           partially observable games spread out too much for the whole disk in 300 steps);
#   None    nothing: the unmasked policy on NoWhereToRun9x8 is there for the refused rows, its masks hold no attack.
# melee8x8Mixed6 has no Resource, Base or Barracks, so HARVEST, RETURN and PRODUCE cannot be set there.
_FIGHT, _ALL = (0, 1, 5), (0, 1, 2, 3, 4, 5)
STEPS = [Step(f"{t}-8x8", t, BASES8 if t == "t5r3" else MELEE8, "masked", 300, False, "disk", _ALL if t == "t5r3" else _FIGHT)
         for t in IDS]
STEPS += [Step(f"{t}-9x8-uniform", t, NOWHERE, "uniform", 200, False, None, ()) for t in IDS]
STEPS += [Step("r5-16x16-po", "r5", "maps/16x16/melee16x16Mixed12.xml", "masked", 300, True, "some", _FIGHT),
          Step("t5r3-16x16-po", "t5r3", "maps/16x16/basesWorkers16x16.xml", "masked", 300, True, "some", _ALL)]


def check_reach(sc, reach):
    """A rollout of STEPS reached what its `reach` and `types` ask for (reach: the Reach its masks were shown to)."""
    c = TABLES[sc.table]
    if sc.reach is None:
        return
    if sc.reach == "disk":
        want = disk(c)
        assert np.array_equal(reach.window, want), \
            f"{sc.id}: attack slots reached\n{reach.window.astype(int)}\nthe table's disk\n{want.astype(int)}"
    else:
        far = disk(c) & ~disk(c, 1)
        assert reach.window.any() and (not c.far or (reach.window & far).any()), \
            f"{sc.id}: attack slots reached\n{reach.window.astype(int)}"
        assert not (reach.window & ~disk(c)).any(), f"{sc.id}: a slot outside the disk\n{reach.window.astype(int)}"
    assert reach.types[list(sc.types)].all(), f"{sc.id}: action-type bits reached {reach.types.astype(int)}"


def oracle_reach(sc):
    """The masked rollout of a STEPS case on the oracle alone (its own Philox rows from its own masks, which
    tests.gpu_checks.rollout proves equal to the kernels') -> Reach."""
    from tests import oracle_py
    from tests.defs import SEED

    c = TABLES[sc.table]
    S = N_SP + N_BOT
    ref = oracle_py.OracleVecClient(N_SP, N_BOT, 2000, [sc.map] * S, seed=GAME_SEED, partial_obs=sc.po,
                                    bot_kinds=[oracle_py.BOT_RANDOM_BIASED] * N_BOT, utt_json=utt_json(sc.table))
    ref.reset()
    reach = Reach(c)
    for step in range(sc.steps):
        m = ref.get_masks(0)
        reach.add(m)
        ref.step(np.stack([oracle_py.policy(m[s], SEED, s, step, 0, c.nt) for s in range(S)]))
    ref.close()
    return reach
