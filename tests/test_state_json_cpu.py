"""The product's own state converters on the CPU (mrts_hostdata.cpp: jsonToBlock, gameToJson, the canonical dump),
reached without a handle through the two internal probes (mrts_internal_state_probe / mrts_internal_dump_probe, beside
them in that file; not in include/mrts.h): a state JSON goes into a zeroed state block and comes back as text, or as
the dump's words.  The reference is the CPU oracle taking in the same text.  No GPU call is made."""
import ctypes
import json

import numpy as np
import pytest

from tests import oracle_py
from tests import state_cases as SC
from tests.state_json_invalid import BASE4X4_JSON, invalid_states
from tests import dumps
from tests.dumps import xy_free

_id = lambda size: f"{size[1]}x{size[0]}"  # noqa: E731


@pytest.fixture(scope="module")
def lib():
    from microrts_amd import _lib

    L = _lib.load()
    I, C, P = ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p
    for f in (L.mrts_internal_state_probe, L.mrts_internal_dump_probe):
        f.argtypes, f.restype = [I, I, I, I, I, I, C, C, P, I, C, I], I
    return L


def probe(f, size, max_units, text, cap, utt_version=1, crs=1, utt_json=None):
    """-> (return value, the bytes / words written, the refusal's text) for a handle of this size as mrts_create sizes it"""
    H, W = size
    mu = min(max_units, H * W) if max_units else H * W
    out = np.zeros(cap, np.int32)
    err = ctypes.create_string_buffer(256)
    n = f(H, W, mu + max(64, mu // 4), mu, utt_version, crs, utt_json, text.encode(), out.ctypes.data_as(ctypes.c_void_p),
          cap * (4 if f.__name__ == "mrts_internal_state_probe" else 1), err, 256)
    return n, out, err.value.decode()


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


def test_probe_refuses_what_a_handle_could_not_be(lib):
    n, _, err = probe(lib.mrts_internal_state_probe, (4, 4), 0, BASE4X4_JSON, 4096, utt_version=4)
    assert n == -22 and "utt_version" in err
    n, _, err = probe(lib.mrts_internal_state_probe, (4, 4), 0, BASE4X4_JSON, 4)  # 16 bytes
    assert n == -28 and err == "buffer too small"
    n, _, err = probe(lib.mrts_internal_state_probe, (4, 4), 3, BASE4X4_JSON, 4096)  # 4 units, max_units 3
    assert n == -28 and "max_units" in err
