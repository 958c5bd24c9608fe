"""State JSON that jsonToBlock must refuse, shared by the GPU test (mrts_set_state_json on a live base4x4 handle,
tests/test_state_json.py) and the CPU test (the internal state probe, tests/test_state_json_cpu.py): what Java would
throw on, and text that is no JSON.  A plain helper module, no fixtures of its own."""
import json

BASE4X4_JSON = ('{"time":0,"pgs":{"width":4,"height":4,"terrain":"0000000000000000","players":[{"ID":0, "resources":5},'
                '{"ID":1, "resources":5}],"units":[{"type":"Resource", "ID":4, "player":-1, "x":0, "y":0, "resources":10, '
                '"hitpoints":1},{"type":"Base", "ID":5, "player":0, "x":1, "y":1, "resources":0, "hitpoints":10},'
                '{"type":"Base", "ID":6, "player":1, "x":3, "y":3, "resources":0, "hitpoints":10},{"type":"Worker", '
                '"ID":7, "player":0, "x":1, "y":0, "resources":0, "hitpoints":1}]},"actions":[]}')
EINVAL = -22


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
    return [(what, json.dumps(x), EINVAL) for what, x in bad] + [("no JSON", "{broken", EINVAL)]
