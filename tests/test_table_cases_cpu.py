"""tests/table_cases.py without a GPU: each table's numbers against the CPU oracle and against the product's own
JSON parser, and what the GPU tests of tests/test_gpu_tables.py rely on reaching, shown on the oracle alone."""
import json

import numpy as np
import pytest

from microrts_amd.vec_client import UnitTypeTable
from tests import oracle_py, table_cases as T
from tests.defs import SEED
from tests.gpu_checks import fm_mixed


@pytest.mark.parametrize("table", T.IDS)
def test_numbers_against_oracle_and_product(table):
    c = T.TABLES[table]
    js = T.utt_json(table)
    assert c.K == 1 + 22 + c.nt + c.R * c.R and c.R in (3, 5) and c.K != 79
    ref = oracle_py.OracleVecClient(2, 0, 100, [T.NOWHERE] * 2, utt_json=js)
    assert (ref.K, ref.H, ref.W) == (c.K, 8, 9)
    ref.close()
    utt = UnitTypeTable.fromJSON(js)  # the product's parser (mrts_utt_json): refuses what mrts_create would
    assert len(utt.TYPES) == c.nt and 2 * utt.getMaxAttackRange() + 1 == c.R
    assert utt.getMoveConflictResolutionStrategy() == c.crs
    assert tuple(u["name"] for u in utt.getUnitTypes() if u["attackRange"] > 1) == c.far
    assert [u["ID"] for u in utt.getUnitTypes()] == list(range(c.nt))
    names = set(utt.TYPES)
    for u in utt.getUnitTypes():
        assert set(u["produces"]) <= names and set(u["producedBy"]) <= names, u["name"]
    assert UnitTypeTable.fromJSON(utt.toJSON()).toJSON() == utt.toJSON()


def test_tables_are_the_issue_s():
    by = {t: {u["name"]: u for u in json.loads(T.utt_json(t))["unitTypes"]} for t in T.IDS}
    assert by["r5"]["Ranged"]["attackRange"] == 2 and by["r3"]["Ranged"]["attackRange"] == 1
    assert list(by["t5r3"]) == list(T.KEEP5) and by["t5r3"]["Barracks"]["produces"] == ["Light"]
    assert by["t8r5"]["Tower"]["attackRange"] == 2 and by["t8r5"]["Worker"]["produces"] == ["Base", "Barracks", "Tower"]
    assert by["t8r5"]["Heavy"]["hp"] == 8  # VERSION_ORIGINAL_FINETUNED
    assert T.disk(T.TABLES["r5"]).sum() == 12 and T.disk(T.TABLES["r3"]).sum() == 4
    c = T.TABLES["t8r5"]
    assert T.atk_base(c) == 31 and T.atk_index(c, -2, 0) == 10 and T.atk_index(c, 2, 2) == 24


@pytest.mark.parametrize("sc", [s for s in T.STEPS if s.reach], ids=[s.id for s in T.STEPS if s.reach])
def test_step_rollouts_reach_their_window(sc):
    """The non-vacuity conditions of tests/test_gpu_tables.py test_step_matches_oracle, on the oracle alone."""
    T.check_reach(sc, T.oracle_reach(sc))


def test_check_reach_can_fail():
    sc = T.STEPS[0]
    r = T.Reach(T.TABLES[sc.table])
    m = np.zeros((1, 1, 1, 55), np.uint8)
    m[..., [1, 2, 6]] = 1
    m[..., 30:] = T.disk(r.c).reshape(-1)
    r.add(m)
    T.check_reach(sc, r)
    r.window[0, 2] = False
    with pytest.raises(AssertionError, match="attack slots reached"):
        T.check_reach(sc, r)
    r.window[0, 2], r.types[5] = True, False
    with pytest.raises(AssertionError, match="action-type bits"):
        T.check_reach(sc, r)


def test_tower_is_built_within_the_compared_steps():
    """test_observation_encodings (t8r5, 8x8) asserts that a Tower (type plane 8) shows in a compared observation."""
    ref = oracle_py.OracleVecClient(8, 0, 2000, [T.BASES8] * 8, seed=3, utt_json=T.utt_json("t8r5"))
    obs, _, _ = ref.reset()
    seen = set()
    for step in range(60):
        m = ref.get_masks(0)
        obs, _, _ = ref.step(np.stack([oracle_py.policy(m[s], SEED, s, step, 0, 8) for s in range(8)]))
        if step + 1 in (10, 30, 60):
            seen |= set(np.unique(obs[:, 3]).tolist())
    ref.close()
    assert 8 in seen, sorted(seen)


@pytest.mark.parametrize("table", ["t8r5", "r5"])
def test_forward_model_evaluations_differ(table):
    """test_forward_model_matches_oracle asks for 5 distinct evaluation values (either player's): the oracle's own playouts give them."""
    n = 16
    ai1, ai2, _, _ = fm_mixed(n)
    ref = oracle_py.OracleForwardModel(n, T.MELEE8, ai1, ai2, seed=21, utt_json=T.utt_json(table))
    seen = set()
    for horizon in (0, 1, 13, 50, 100):
        for g in range(n):
            ref.playout(g, horizon)
            seen |= {float(ref.evaluate(g, 0)), float(ref.evaluate(g, 1))}
    ref.close()
    assert len(seen) >= 5, sorted(seen)


def test_fused_rollout_meets_enemies_beyond_one_cell(tmp_path):
    """test_fused_forms_equal_the_per_step_handle (r5) asks for an attack slot more than one cell away in a compared
    mask: the masks after steps 1, 2, 7, 8, 9, 14, 19, 20, 21, 26, ..., 56 and 60 of its rollout, on the oracle."""
    from tests.combat_maps import mixed_maps

    c, S = T.TABLES["r5"], 8
    ref = oracle_py.OracleVecClient(S, 0, 300, mixed_maps(tmp_path, S), seed=6, utt_json=T.utt_json("r5"))
    ref.reset()
    window = np.zeros((c.R, c.R), bool)
    compared = {1, 2, 7, 8, 9, 14, 19, 20, 60} | set(range(21, 60, 5))
    for step in range(61):
        m = ref.get_masks(0)
        if step in compared:
            window |= m[..., T.atk_base(c):].reshape(-1, c.R, c.R).any(axis=0)
        ref.step(np.stack([oracle_py.policy(m[s], SEED, s, step, 0, c.nt) for s in range(S)]))
    ref.close()
    assert (window & ~T.disk(c, 1)).any(), window.astype(int)
