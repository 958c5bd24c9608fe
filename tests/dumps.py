"""The canonical state dump, read in one place.  Test infrastructure only.

mrts_get_state and the oracle's dumpState emit the same int32 words:

    time, 2, res0, res1,
    nu, nu x (type, player, x, y, hp, resources)                                  units in list order
    na, na x (unit index, action type, parameter, x, y, unit type or -1, time)    assignments in issue order

No other file of tests/ or tools/ does index arithmetic on a dump."""
import collections

import numpy as np

UNIT_WORDS, ASSIGN_WORDS = 6, 7
ATTACK = 5  # the one action type whose x / y are read (UnitAction.ATTACK_LOCATION)

State = collections.namedtuple("State", "time res units assign")


def _units_at(d):
    return 5, 5 + UNIT_WORDS * int(d[4])


def _assign_at(d):
    b = _units_at(d)[1]
    return b + 1, b + 1 + ASSIGN_WORDS * int(d[b])


def parse(dump):
    """dump -> State(time, (res0, res1), units int32 [nu][6], assign int32 [na][7]); the arrays are copies."""
    d = np.asarray(dump, np.int32)
    assert len(d) >= 6 and d[1] == 2, f"not a state dump of two players: {d[:6].tolist()} ... ({len(d)} words)"
    u0, u1 = _units_at(d)
    assert u1 < len(d), f"dump of {len(d)} words cannot hold its {int(d[4])} units"
    a0, a1 = _assign_at(d)
    assert a1 == len(d), f"dump of {len(d)} words, but {int(d[4])} units and {int(d[u1])} assignments end at word {a1}"
    return State(int(d[0]), (int(d[2]), int(d[3])), d[u0:u1].reshape(-1, UNIT_WORDS).copy(),
                 d[a0:a1].reshape(-1, ASSIGN_WORDS).copy())


def build(time, res, units, assign):
    """The inverse of parse."""
    units, assign = np.asarray(units, np.int32).reshape(-1, UNIT_WORDS), np.asarray(assign, np.int32).reshape(-1, ASSIGN_WORDS)
    return np.concatenate([[time, 2, res[0], res[1], len(units)], units.ravel(), [len(assign)], assign.ravel()]).astype(np.int32)


def n_units(dump):
    return int(dump[4])


def n_assign(dump):
    return int(dump[_units_at(dump)[1]])


def live_units(dump):
    """The unit list [nu][6]: (type, player, x, y, hp, resources)."""
    return parse(dump).units


def assignment_of(dump, k):
    """(assignment row of unit k, its place in the issue order), or None for a unit that holds none."""
    for i, a in enumerate(parse(dump).assign):
        if a[0] == k:
            return a, i
    return None


def xy_free(dump):
    """A canonical dump with x/y of non-attack assignments zeroed: UnitAction.fromJSON leaves them at
    DIRECTION_NONE (-1) where a decoded action holds 0; only ATTACK_LOCATION reads them."""
    d = np.array(dump)
    a0, a1 = _assign_at(d)
    rows = d[a0:a1].reshape(-1, ASSIGN_WORDS)  # a view: the writes below land in d
    rows[rows[:, 1] != ATTACK, 3:5] = 0
    return d


def difference(a, b, around=14):
    """Where two dumps differ, for an assertion message: the first differing word and the words around it."""
    n = min(len(a), len(b))
    ne = np.asarray(a[:n]) != np.asarray(b[:n])
    i = int(np.argmax(ne)) if ne.any() else n
    return (f"at word {i} (len {len(a)} vs {len(b)}):\n gpu {np.asarray(a[max(0, i - around):i + around]).tolist()}"
            f"\n ref {np.asarray(b[max(0, i - around):i + around]).tolist()}\n gpu {np.asarray(a).tolist()}"
            f"\n ref {np.asarray(b).tolist()}")
