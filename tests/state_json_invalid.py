"""State JSON that jsonToBlock must refuse, shared by the GPU test (mrts_set_state_json on a live base4x4 handle,
tests/test_state_json.py) and the CPU test (the internal state probe, tests/test_state_json_cpu.py): what Java would
throw on, and text that is no JSON.  A plain helper module, no fixtures of its own."""
import json

from tests.defs import DOWN, HARVEST, LEFT, MOVE, PRODUCE, RETURN, RIGHT, UP

BASE4X4_JSON = ('{"time":0,"pgs":{"width":4,"height":4,"terrain":"0000000000000000","players":[{"ID":0, "resources":5},'
                '{"ID":1, "resources":5}],"units":[{"type":"Resource", "ID":4, "player":-1, "x":0, "y":0, "resources":10, '
                '"hitpoints":1},{"type":"Base", "ID":5, "player":0, "x":1, "y":1, "resources":0, "hitpoints":10},'
                '{"type":"Base", "ID":6, "player":1, "x":3, "y":3, "resources":0, "hitpoints":10},{"type":"Worker", '
                '"ID":7, "player":0, "x":1, "y":0, "resources":0, "hitpoints":1}]},"actions":[]}')
EINVAL, ENOTSUP = -22, -95
# BASE4X4_JSON's units by list position: the Resource at (0, 0), player 0's Base at (1, 1), player 1's Base at (3, 3)
# and player 0's Worker at (1, 0)
BASE0, BASE1, WORKER = 1, 2, 3


def with_action(unit, x, y, kind, direction, time=0):
    """BASE4X4_JSON with the unit at list position `unit` standing at (x, y) and holding an action of this kind
    and direction (a PRODUCE makes a Worker), as a dict; unit IDs are list positions, as the build writes them"""
    b = json.loads(BASE4X4_JSON)
    for i, v in enumerate(b["pgs"]["units"]):
        v["ID"] = i
    u = b["pgs"]["units"][unit]
    u["x"], u["y"] = x, y
    a = {"type": kind, "parameter": direction}
    if kind == PRODUCE:
        a["unitType"] = "Worker"
    b["actions"] = [{"ID": u["ID"], "time": time, "action": a}]
    return b


def edge_states():
    """[(what, text)] that jsonToBlock must keep: a HARVEST or RETURN that points off the map (UnitAction.execute
    tests the cell first, Java and the kernels alike), and a MOVE or PRODUCE along the edge that stays on the map."""
    ok = [("harvest off the top edge", with_action(WORKER, 2, 0, HARVEST, UP)),
          ("return off the left edge", with_action(WORKER, 0, 2, RETURN, LEFT)),
          ("harvest off the bottom edge", with_action(WORKER, 1, 3, HARVEST, DOWN)),
          ("return off the right edge", with_action(WORKER, 3, 1, RETURN, RIGHT)),
          ("move along the top edge", with_action(WORKER, 2, 0, MOVE, RIGHT)),
          ("move along the left edge", with_action(WORKER, 0, 2, MOVE, DOWN)),
          ("move into the corner", with_action(WORKER, 2, 3, MOVE, LEFT)),
          ("produce along the bottom edge", with_action(BASE1, 3, 3, PRODUCE, LEFT)),
          ("produce along the right edge", with_action(BASE1, 3, 3, PRODUCE, UP))]
    return [(what, json.dumps(x)) for what, x in ok]


def invalid_states():
    """[(what, text, the error code it is refused with)] for a 4x4 handle with the original unit-type table"""
    bad = []
    b = json.loads(BASE4X4_JSON)
    b["pgs"]["width"] = 5
    bad.append(("size differs", b))
    b = json.loads(BASE4X4_JSON)
    b["pgs"]["units"][1]["x"] = 0
    b["pgs"]["units"][1]["y"] = 0
    bad.append(("two units in a cell", b))
    b = json.loads(BASE4X4_JSON)
    b["actions"] = [{"ID": 99, "time": 0, "action": {"type": 0, "parameter": 10}}]
    bad.append(("unknown ID", b))
    b = json.loads(BASE4X4_JSON)
    b["pgs"]["units"][0]["type"] = "Dragon"
    bad.append(("unknown unit type", b))
    # a MOVE or PRODUCE under way whose target cell is off the map: UnitAction.execute writes that cell unguarded
    off = [("move off the top edge", with_action(WORKER, 1, 0, MOVE, UP)),
           ("move off the right edge", with_action(WORKER, 3, 1, MOVE, RIGHT)),
           ("move off the bottom edge", with_action(WORKER, 1, 3, MOVE, DOWN)),
           ("move off the left edge", with_action(WORKER, 0, 2, MOVE, LEFT)),
           ("produce off the right edge", with_action(BASE1, 3, 3, PRODUCE, RIGHT)),
           ("produce off the bottom edge", with_action(BASE1, 3, 3, PRODUCE, DOWN))]
    return [(what, json.dumps(x), EINVAL) for what, x in bad] + [(what, json.dumps(x), ENOTSUP) for what, x in off] + \
        [("no JSON", "{broken", EINVAL)]
