"""tests.state_cases on the oracle alone: the state source of tests/test_gpu_every_shape.py.

* every picked entry of every recorded game survives dump -> GameState.toJSON text -> set_state_json ->
  dump (under dumps.xy_free: UnitAction.fromJSON leaves x / y of non-attack actions at -1);
* the case list the GPU test imports reaches what it is there for.  These are conditions, asserted so
  that a later change to the generator cannot empty the GPU test silently: on a miss, change the
  generator's parameters or seed for that size, not the condition;
* why the GPU test compares reversed Java rows with the oracle's step_rows and not with the grid step.
"""
import json

import numpy as np
import pytest

from tests import oracle_py
from tests import state_cases as SC
from tests.dumps import xy_free

_id = lambda size: f"{size[1]}x{size[0]}"  # noqa: E731


def test_the_17_sizes():
    assert len(SC.SIZES) == 17 and SC.SIZES[0] == (4, 4) and SC.SIZES[-1] == (128, 128)
    assert {(8, 9), (8, 16), (12, 14), (12, 16), (14, 15), (96, 128), (128, 96), (112, 128)} <= set(SC.SIZES)
    assert set(SC.BOT_SIZES) <= set(SC.SIZES)


@pytest.mark.parametrize("size", SC.SIZES, ids=_id)
def test_trace_states_round_trip(size):
    st = SC.trace_states(size)
    tm = SC.templates(size)
    assert len(st) >= 2 * len(SC.GROUPS[size])
    maps = sorted(tm)
    ref = oracle_py.OracleVecClient(2 * len(maps), 0, 2000, [m for m in maps for _ in range(2)])
    ref.reset()
    for mp, fx, k, dump in st:
        s = 2 * maps.index(mp)
        ref.set_state_json(s, SC.dump_to_json(tm[mp], dump))
        assert np.array_equal(xy_free(ref.dump(s)), xy_free(dump)), f"{fx} entry {k}"
        assert ref.env_steps(s) == 0
    ref.close()


@pytest.mark.parametrize("size", SC.SIZES, ids=_id)
def test_cases_reach_what_they_are_for(size):
    H, W = size
    c = SC.case(size)
    n = len(c["states"])
    assert n >= 1 and len(c["maps"]) == 2 * n and c["max_steps"] < c["steps"]
    assert n <= (8 if H * W > 64 * 64 else 24)
    assert (c["max_units"] == 1024) == (H * W > 64 * 64)
    for g, j in enumerate(c["states"]):
        pgs = json.loads(j)["pgs"]
        assert (pgs["height"], pgs["width"]) == size
        assert c["crowded"][g] or len(pgs["units"]) == c["trace_units"][g]  # a full 4x4 map takes no crowd
    assert any(len(json.loads(j)["pgs"]["units"]) > t for j, t in zip(c["states"], c["trace_units"]))
    r = SC.oracle_run(c)  # raises what Java would throw (two units in a cell)
    assert r["types"] == set(range(7)), f"unit types {sorted(r['types'])}"
    assert r["owners"] == {-1, 0, 1}
    if H * W >= 144:
        assert r["most_units"] > 64, f"no game with more than 64 units ({r['most_units']})"
    # BroodWar maps (all of those above 64x64 cells) close row H-1 with wall: the last open row stands in
    assert c["edge_row"] == H - 1 or (H * W > 64 * 64 and c["edge_row"] == H - 2)
    assert r["last_col"] > 0, "no candidate cell in the last column"
    assert r["last_row"] > 0, "no candidate cell in the last row"
    assert r["attack_bits"] > 0, "no attack-window mask bit"
    assert r["deaths"] > 0, "no unit died"
    assert r["resets"] >= n, "not every game reset inside a step"
    assert r["errors"] == 0, "a step made Java print an error (the kernels' error flags would be set)"


@pytest.mark.parametrize("size", SC.BOT_SIZES, ids=_id)
def test_bot_cases(size):
    c = SC.bot_case(size)
    n = len(c["states"])
    assert 2 <= n <= 8 and len(c["maps"]) == n and c["players"] == [0, 1] * (n // 2) and any(c["crowded"])
    ref = oracle_py.OracleVecClient(0, n, c["max_steps"], c["maps"], seed=SC.GAME_SEED,
                                    bot_kinds=[oracle_py.BOT_RANDOM_BIASED] * n)
    ref.reset(c["players"])
    for g, j in enumerate(c["states"]):
        ref.set_state_json(g, j)
    resets = 0
    for step in range(c["steps"]):
        m = ref.get_masks(0)
        _, _, done = ref.step(np.stack([oracle_py.policy(m[s], SC.SEED, s, step, 0) for s in range(n)]), c["players"])
        resets += int(done.sum())
    assert resets >= n
    ref.close()


def test_reversed_rows_are_another_step():
    """PlayerAction.fromVectorAction reads the rows in list order and refuses a row whose cell or resources
    an earlier row of the same player claimed: on the crowded 8x8 games the reversed list is another step
    than the grid's (rows in ascending order), while the ascending list is the grid's step."""
    c = SC.case((8, 8))
    S = 2 * len(c["states"])
    refs = [oracle_py.OracleVecClient(S, 0, c["max_steps"], c["maps"], seed=SC.GAME_SEED) for _ in range(3)]
    for r in refs:
        r.reset()
        for g, j in enumerate(c["states"]):
            r.set_state_json(2 * g, j)
    m = refs[0].get_masks(0)
    acts = np.stack([oracle_py.policy(m[s], SC.SEED, s, 0, 0) for s in range(S)])
    refs[0].step(acts)
    refs[1].step_rows(SC.java_rows(acts, reverse=False))
    refs[2].step_rows(SC.java_rows(acts, reverse=True))
    assert np.array_equal(refs[0].obs, refs[1].obs) and np.array_equal(refs[0].get_masks(0), refs[1].get_masks(0))
    assert not np.array_equal(refs[0].obs, refs[2].obs)
    for r in refs:
        r.close()
