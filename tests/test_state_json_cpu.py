"""The product's own state converters on the CPU (mrts_hostdata.cpp: jsonToBlock, gameToJson, the canonical dump),
reached without a handle through the two internal probes (mrts_internal_state_probe / mrts_internal_dump_probe, beside
them in that file; not in include/mrts.h): a state JSON goes into a zeroed state block and comes back as text, or as
the dump's words.  The reference is the CPU oracle taking in the same text.  No GPU call is made."""
import json

import numpy as np
import pytest

from tests import oracle_py
from tests import state_cases as SC
from tests.state_json_invalid import BASE4X4_JSON, EINVAL, ENOTSUP, edge_states, invalid_states
from tests import dumps
from tests.dumps import xy_free

_id = lambda size: f"{size[1]}x{size[0]}"  # noqa: E731


@pytest.fixture(scope="module")
def lib():
    from microrts_amd import _lib

    return _lib.load()


def probe(f, size, max_units, text, cap, utt_version=1, crs=1, utt_json=None):
    """-> (return value, the bytes / words written, the refusal's text) for a handle of this size as mrts_create sizes it"""
    return SC.state_probe(f.__name__, size, max_units, text, cap, utt_version, crs, utt_json)


@pytest.mark.parametrize("size", SC.SIZES, ids=_id)
def test_round_trip_equals_the_oracles(lib, size):
    """One state per map size (a crowded one where the size has one: every unit type, both owners, assignments under
    way): the product's text after the round trip is the oracle's toJSON text of the same state, byte for byte, and
    its dump is the oracle's (under dumps.xy_free, as everywhere a dump follows fromJSON: UnitAction.fromJSON leaves
    x / y of a non-attack action at -1 where the kernels' decoded action holds 0)."""
    c = SC.case(size)
    g = 1 if len(c["states"]) > 1 else 0
    text, mp = c["states"][g], c["maps"][2 * g]
    ref = oracle_py.OracleVecClient(2, 0, 2000, [mp] * 2)
    ref.reset()
    ref.set_state_json(0, text)
    want_json, want_dump = ref.state_json(0), ref.dump(0)
    ref.close()
    assert json.loads(want_json)["pgs"]["units"], "an empty state proves nothing"
    n, out, err = probe(lib.mrts_internal_state_probe, size, c["max_units"], text, 1 << 18)
    assert n > 0, err
    assert out.tobytes()[:n].decode() == want_json
    n, out, err = probe(lib.mrts_internal_dump_probe, size, c["max_units"], text, 1 << 18)
    assert n > 0, err
    assert len(want_dump) == n and np.array_equal(xy_free(out[:n]), xy_free(want_dump))
    got, want = dumps.parse(out[:n]), dumps.parse(want_dump)
    assert got[:2] == want[:2] and np.array_equal(got.units, want.units), "time, players and units exactly"


def test_invalid_states_are_refused_with_the_gpu_paths_codes(lib):
    n, out, err = probe(lib.mrts_internal_state_probe, (4, 4), 0, BASE4X4_JSON, 4096)
    assert n > 0 and json.loads(out.tobytes()[:n].decode())["pgs"]["units"][3]["type"] == "Worker", err
    for what, text, code in invalid_states():
        for f in (lib.mrts_internal_state_probe, lib.mrts_internal_dump_probe):
            n, _, err = probe(f, (4, 4), 0, text, 4096)
            assert n == code and err.startswith("state json:"), (what, n, err)


def test_every_invalid_state_keeps_its_own_code():
    """The list's codes case by case: what Java would throw on is EINVAL, an off-map MOVE / PRODUCE target (what
    this build cannot hold) ENOTSUP with a text that names it."""
    bad = invalid_states()
    assert [(what, code) for what, _, code in bad if not what.startswith(("move off", "produce off"))] == \
        [("size differs", EINVAL), ("two units in a cell", EINVAL), ("unknown ID", EINVAL), ("unknown unit type", EINVAL),
         ("no JSON", EINVAL)]
    off = [(what, text) for what, text, code in bad if code == ENOTSUP]
    assert [what for what, _ in off] == ["move off the top edge", "move off the right edge", "move off the bottom edge",
                                         "move off the left edge", "produce off the right edge", "produce off the bottom edge"]
    assert len(off) + 5 == len(bad)


def test_off_map_targets_are_refused_by_both_sides(lib):
    """An in-flight MOVE or PRODUCE whose target cell is off the map: jsonToBlock and the oracle's set_state_json
    refuse the same states with the same words, and the oracle's game stays what it was."""
    ref = oracle_py.OracleVecClient(2, 0, 2000, ["maps/4x4/base4x4.xml"] * 2)
    ref.reset()
    before = ref.state_json(0)
    for what, text, code in invalid_states():
        if code != ENOTSUP:
            continue
        kind = what.split()[0]
        n, _, err = probe(lib.mrts_internal_state_probe, (4, 4), 0, text, 4096)
        assert n == ENOTSUP and err == f"state json: {kind} target off the map", (what, n, err)
        with pytest.raises(RuntimeError, match=f"state json: {kind} target off the map"):
            ref.set_state_json(0, text)
        assert ref.state_json(0) == before, what
    ref.close()


def test_edge_actions_that_stay_legal_round_trip(lib):
    """HARVEST / RETURN pointing off the map and MOVE / PRODUCE along the edge are kept by both sides: the product's
    text and dump after the round trip are the oracle's, and the oracle then runs the action to its end without an
    error (the off-map HARVEST / RETURN does nothing, like Java's)."""
    ref = oracle_py.OracleVecClient(2, 0, 2000, ["maps/4x4/base4x4.xml"] * 2)
    ref.reset()
    cases = edge_states()
    assert {json.loads(t)["actions"][0]["action"]["type"] for _, t in cases} == {1, 2, 3, 4}
    for what, text in cases:
        ref.set_state_json(0, text)
        want_json, want_dump = ref.state_json(0), ref.dump(0)
        assert len(json.loads(want_json)["actions"]) == 1, what
        n, out, err = probe(lib.mrts_internal_state_probe, (4, 4), 0, text, 4096)
        assert n > 0, (what, err)
        assert out.tobytes()[:n].decode() == want_json, what
        n, out, err = probe(lib.mrts_internal_dump_probe, (4, 4), 0, text, 4096)
        assert n == len(want_dump) and np.array_equal(xy_free(out[:n]), xy_free(want_dump)), (what, err)
        for _ in range(60):  # past the longest of them, the Worker's production (50 cycles)
            ref.step(np.zeros((2, 16, 7), np.int32))
        assert not json.loads(ref.state_json(0))["actions"] or what.startswith("produce"), what
        assert ref.L.oref_errors(ref.h, 0) == 0, what
    ref.close()


def test_probe_refuses_what_a_handle_could_not_be(lib):
    n, _, err = probe(lib.mrts_internal_state_probe, (4, 4), 0, BASE4X4_JSON, 4096, utt_version=4)
    assert n == -22 and "utt_version" in err
    n, _, err = probe(lib.mrts_internal_state_probe, (4, 4), 0, BASE4X4_JSON, 4)  # 16 bytes
    assert n == -28 and err == "buffer too small"
    n, _, err = probe(lib.mrts_internal_state_probe, (4, 4), 3, BASE4X4_JSON, 4096)  # 4 units, max_units 3
    assert n == -28 and "max_units" in err
