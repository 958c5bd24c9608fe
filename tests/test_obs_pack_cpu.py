"""Packed observation rows without a GPU (include/mrts.h "Packed observation rows"): the header and the binding name
the entry points, the word-count formula of mrts_internal.h is the documented one, and the numpy packer of
tests/obs_pack_ref.py (the GPU tests' reference) round-trips oracle observations and flags the synthetic rows as
the layout says."""
import os

import numpy as np
import pytest

from microrts_amd import _lib
from tests import obs_pack_ref as OR
from tests.headers import header_symbols, internal_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["mrts_obs_packed_words", "mrts_obs_pack_dev", "mrts_obs_unpack_dev", "mrts_obs_onehot_packed_dev",
                "mrts_obs_packed_status"]


def test_header_and_binding_name_the_entry_points():
    hdr = header_symbols()
    for name in ENTRY_POINTS:
        assert name in hdr, f"{name} is not declared in include/mrts.h"
        assert name in _lib.EXPORTS, f"{name} is not in _lib.EXPORTS"
    assert "Packed observation rows" in open(os.path.join(ROOT, "include", "mrts.h")).read()


# 1 + 2 * cap + (C - 5) * ceil(H*W / 32); (8, 32x32, 128) is 1 + 256 + 3 * 32
@pytest.mark.parametrize("C,HW,cap,want", [(6, 256, 128, 265), (8, 1024, 128, 353), (6, 72, 72, 148)])
def test_word_count_formula(C, HW, cap, want):
    f = internal_header()["obsPackedWords"]
    assert want == 1 + 2 * cap + (C - 5) * -(-HW // 32)
    assert f(C, HW, cap) == want == OR.words(C, HW, cap)


@pytest.mark.parametrize("po", [False, True], ids=["full", "po"])
@pytest.mark.parametrize("shape", ["8x8", "16x16"])
def test_numpy_packer_round_trips_oracle_observations(shape, po):
    from tests.oracle_py import OracleVecClient

    S = 4
    env = OracleVecClient(S, 0, 2000, [f"maps/{shape}/basesWorkers{shape}.xml"] * S, partial_obs=po, seed=3)
    obs = [env.reset()[0]]
    for k in range(30):
        env.rollout_policy(1, 11, 0, k)
        obs.append(env.obs.copy())
    env.close()
    obs = np.concatenate(obs)
    HW = env.H * env.W
    assert env.C == (8 if po else 6) and (obs[1:] != obs[:-1]).any()
    rows = OR.pack(obs, HW)
    assert rows.dtype == np.uint32 and rows.shape == (len(obs), OR.words(env.C, HW, HW))
    assert not (rows[:, 0] & OR.LOSSY).any(), "a row of the oracle's is flagged at cap = H*W"
    assert (rows[:, 0] > 0).all() and rows[:, 0].max() < HW
    assert np.array_equal(OR.unpack(rows, env.C, env.H, env.W, HW), obs)
    # the default cap holds these rollouts too, and a cut row keeps its true count and its first cells
    cap = int(rows[:, 0].max()) - 1
    cut = OR.pack(obs, cap)
    over = rows[:, 0] > cap
    assert over.any() and np.array_equal(cut[:, 0], rows[:, 0] | np.where(over, OR.LOSSY, 0).astype(np.uint32))
    assert np.array_equal(cut[:, 1:1 + 2 * cap], rows[:, 1:1 + 2 * cap]) and np.array_equal(cut[:, 1 + 2 * cap:], rows[:, 1 + 2 * HW:])


@pytest.mark.parametrize("H,W,C", [(4, 4, 6), (9, 8, 8), (16, 16, 6), (32, 32, 8)])
def test_synthetic_rows_carry_their_flags_and_counts(H, W, C):
    HW, cap = H * W, OR.synthetic_cap(H, W)
    obs, names, info = OR.synthetic_rows(H, W, C, seed=HW)
    assert len(set(names)) == len(names) == len(obs)
    at = {k: i for i, k in enumerate(names)}
    assert ("cells_63_64" in at) == (HW > 64) and ("cells_255_256" in at) == (HW > 256)
    count = {"empty": 0, "cell_0": 1, "cell_last": 1, "exactly_cap": cap, "cap_plus_1": cap + 1, "every_cell": HW,
             "only_plane_4": 1, "terrain_2": 1}
    for c, rows in ((cap, OR.pack(obs, cap)), (HW, OR.pack(obs, HW)), (1, OR.pack(obs, 1))):
        n, lossy = rows[:, 0] & (OR.LOSSY - 1), (rows[:, 0] & OR.LOSSY) != 0
        for k, v in count.items():
            assert n[at[k]] == v, (k, c)
        assert np.array_equal(n, [info[k][0] for k in names]), "word 0 keeps the true count"
        assert np.array_equal(lossy, OR.flagged(info, names, c)), c
        back = OR.unpack(rows, C, H, W, c)
        for i, k in enumerate(names):
            if not lossy[i]:
                assert np.array_equal(back[i], obs[i]), (k, c)
        # a kept cell's words are zero past the last kept one
        for i in range(len(names)):
            kept = min(int(n[i]), c)
            assert not rows[i, 1 + 2 * kept:1 + 2 * c].any()
    rows = OR.pack(obs, cap)
    lossy = (rows[:, 0] & OR.LOSSY) != 0
    exact = ["empty", "cell_0", "cell_last", "exactly_cap", "only_plane_4", "hp_-1", "hp_-32768", "hp_32767", "res_65535",
             "owner_3", "action_7", "type_31"]
    clamped = ["hp_32768", "hp_-32769", "res_65536", "res_-1", "owner_4", "action_8", "type_32"]
    assert not lossy[[at[k] for k in exact]].any() and lossy[[at[k] for k in clamped + ["cap_plus_1", "every_cell", "terrain_2"]]].all()
    assert not ((OR.pack(obs, HW)[:, 0] & OR.LOSSY) != 0)[at["every_cell"]]
    # clamped to the field's range: the one-hot encoding does not see it
    back = OR.unpack(rows, C, H, W, cap)
    c = HW // 3
    want = {"hp_32768": (0, 32767), "hp_-32769": (0, -32768), "res_65536": (1, 65535), "res_-1": (1, 0), "owner_4": (2, 3),
            "action_8": (4, 7), "type_32": (3, 31)}
    for k, (p, v) in want.items():
        assert back[at[k]].reshape(C, HW)[p, c] == v, k
    sel = [at[k] for k in clamped + ["terrain_2"]]
    assert np.array_equal(OR.onehot(back[sel], 7), OR.onehot(obs[sel], 7))
    # the stored words of one cell: cell | owner << 16 | action << 18 | type << 21, (hp & 0xFFFF) | resources << 16
    r = rows[at["cell_last"]]
    assert r[1] == (HW - 1) | 2 << 16 | 5 << 18 | 6 << 21 and r[2] == 4 | 7 << 16
    assert rows[at["hp_-1"], 2] == 0xFFFF
