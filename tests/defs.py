"""The game's constants and small encoders, once for the whole suite.  Test infrastructure only.

Unit type ids (UnitTypeTable.java:104-289), action types (UnitAction.java:31-60), directions (up 0, right 1,
down 2, left 3), hit points and costs of UnitTypeTable VERSION_ORIGINAL, the attack index of the 7x7 window
((3 + dy) * 7 + (3 + dx): maxAttackRadius 7, JNIGridnetClient.java:125), a Java action row, the suite's policy
seed and the one writer of the reference's map XML (PhysicalGameState.java:700-726)."""

NONE, MOVE, HARVEST, RETURN, PRODUCE, ATTACK = range(6)
RESOURCE, BASE, BARRACKS, WORKER, LIGHT, HEAVY, RANGED = range(7)
UP, RIGHT, DOWN, LEFT = range(4)
DX, DY = (0, 1, 0, -1), (-1, 0, 1, 0)  # UnitAction.DIRECTION_OFFSET_X/Y
NAMES = {RESOURCE: "Resource", BASE: "Base", BARRACKS: "Barracks", WORKER: "Worker", LIGHT: "Light",
         HEAVY: "Heavy", RANGED: "Ranged"}
HP = {RESOURCE: 1, BASE: 10, BARRACKS: 4, WORKER: 1, LIGHT: 4, HEAVY: 4, RANGED: 1}
COST = {RESOURCE: 1, BASE: 10, BARRACKS: 5, WORKER: 1, LIGHT: 2, HEAVY: 2, RANGED: 2}

SEED = 0x5EEDC0DE  # the policy seed of every rollout in the suite


def atk(dx, dy):
    return (3 + dy) * 7 + (3 + dx)


def row(pos, t=NONE, move=0, harvest=0, ret=0, pdir=0, ptype=0, attack=0):
    """A Java action row [pos, type, move dir, harvest dir, return dir, produce dir, produce type, attack index]."""
    return [pos, t, move, harvest, ret, pdir, ptype, attack]


def write_map(path, W, H, units, walls=(), res=(5, 5)):
    """units: (type, player, x, y[, resources[, hp]]) in list order."""
    terr = ["0"] * (W * H)
    for x, y in walls:
        terr[y * W + x] = "1"
    lines = [f'<rts.PhysicalGameState width="{W}" height="{H}">', f"  <terrain>{''.join(terr)}</terrain>", "  <players>"]
    for i, r in enumerate(res):
        lines += [f'    <rts.Player ID="{i}" resources="{r}">', "    </rts.Player>"]
    lines += ["  </players>", "  <units>"]
    for i, u in enumerate(units):
        t, p, x, y = u[:4]
        r = u[4] if len(u) > 4 else 0
        hp = u[5] if len(u) > 5 else HP[t]
        lines += [f'    <rts.units.Unit type="{NAMES[t]}" ID="{100 + i}" player="{p}" x="{x}" y="{y}" resources="{r}" '
                  f'hitpoints="{hp}" >', "    </rts.units.Unit>"]
    lines += ["  </units>", "</rts.PhysicalGameState>"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return str(path)
