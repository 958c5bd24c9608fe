"""Unit-type tables whose mask layout differs from the built-in K = 79 (tests/table_cases.py: R = 3 or 5, 5 to 8
types) through every output path but the policy head (tests/test_gpu_policy_head*.py) and the hand-derived KATs
(tests/test_kats.py): the step against the oracle, the fused forms against the per-step handle, the uniform policy,
the observation encodings, the forward model, checkpoints and the LightRush opponent.

Every one of these tables runs the generic step kernel (only K = 79 has compile-time instances), the `pv / R`
arm of the attack-index decode and mask windows that lie in other words of the mask row than the 7x7 one."""
import json

import numpy as np
import pytest

from tests import dumps, obs_pack_ref as OR, oracle_py, table_cases as T
from tests.combat_maps import ALL_RFS, mixed_maps
from tests.defs import SEED
from tests.gpu_checks import encode_obs_np, fm_compare, fm_mixed, rollout
from tests.gpu_support import assert_same_outputs, same, torch_gpu

pytestmark = pytest.mark.gpu

M16 = "maps/16x16/basesWorkers16x16.xml"


def _utt(table):
    from microrts_amd import UnitTypeTable

    return UnitTypeTable.fromJSON(T.utt_json(table))


def _env(table, n_sp, n_bot, maps, **kw):
    torch_gpu()
    from microrts_amd import DeviceVecEnv

    env = DeviceVecEnv(n_sp, n_bot, kw.pop("max_steps", 2000), maps, utt=_utt(table), **kw)
    c = T.TABLES[table]
    assert env.dims[4] == c.K and env.actions.shape[-1] == 7 and (env.masks is None or env.masks.shape[-1] == c.K)
    assert not env.multi_step_capable, f"{table}: only the K = 79 instances run several steps per launch"
    return env


@pytest.mark.parametrize("table", T.IDS)
@pytest.mark.parametrize("mp", [T.BASES8, M16], ids=["8x8", "16x16"])
def test_no_multi_step_launches(table, mp):
    """env.multi_step_capable is False under every table of the list, on the square self-play shapes that have
    multi-step instances under the built-in table (True there: the assertion can fail), with and without masks."""
    from microrts_amd import DeviceVecEnv

    for with_masks in (True, False):
        env = _env(table, 4, 0, [mp] * 4, with_masks=with_masks)  # (asserts it)
        assert not env.multi_step_capable and not env.fused_multi_step
        env.close()
    env = DeviceVecEnv(4, 0, 2000, [mp] * 4)
    assert env.multi_step_capable
    env.close()


# ------------------------------------------------------------------ the step against the oracle
@pytest.mark.parametrize("sc", T.STEPS, ids=[s.id for s in T.STEPS])
def test_step_matches_oracle(sc):
    """tests.gpu_checks.rollout, one launch per step, every reward function: masks before every step, the policy
    kernel's rows, observations, rewards and dones after it, every state every 25 steps — 8 self-play slots and 2
    agent-vs-RandomBiasedAI envs.  The oracle's masks of the same rollout reached what tests.table_cases.STEPS says."""
    c = T.TABLES[sc.table]
    reach = T.Reach(c)
    rollout.nonzero = np.zeros(len(ALL_RFS), bool)
    flags = rollout([sc.map] * (T.N_SP + T.N_BOT), T.N_SP, T.N_BOT, steps=sc.steps, policy=sc.policy, partial_obs=sc.po,
                    bots=["RandomBiasedAI"] * T.N_BOT, rfs=ALL_RFS, utt_json=T.utt_json(sc.table), dump_every=25,
                    seed=T.GAME_SEED, reach=reach)
    assert not flags.any(), f"error flags {flags}"
    T.check_reach(sc, reach)


@pytest.mark.parametrize("table", ["r5", "t5r3"])
def test_fused_forms_equal_the_per_step_handle(table, tmp_path):
    """step_fused and rollout_fused against step + random_policy, rollout_uniform (both forms) against uniform_policy
    + step: byte-equal outputs, masks, actions and states over 60 steps on handles of a non-built-in table.  r5 on
    16x16: tests.combat_maps' arena games (Heavy and Ranged against Worker and Light, four cells apart: the melee
    maps' armies do not meet within 60 steps) beside melee16x16Mixed12 games; t5r3 on basesWorkers8x8."""
    torch_gpu()
    n = 8
    c = T.TABLES[table]
    maps = mixed_maps(tmp_path, n) if table == "r5" else [T.BASES8] * n
    mk = lambda **kw: _env(table, n, 0, maps, seed=6, max_steps=300, **kw)  # noqa: E731
    A, B, C = mk(), mk(), mk()
    for e in (A, B, C):
        e.reset()
        e.random_policy(SEED, 0)
    k, window = 0, np.zeros((c.R, c.R), bool)
    for chunk in (1, 7, 12, 40):
        for i in range(chunk):
            A.step()
            A.random_policy(SEED, k + i + 1)
            B.step_fused(SEED, k + i + 1)
            if i % 5 == 0:
                assert_same_outputs(A, B, f"step_fused after {k + i + 1}")
                window |= A.masks[..., T.atk_base(c):].ne(0).reshape(-1, c.R, c.R).any(0).cpu().numpy()
        C.rollout_fused(SEED, k + 1, chunk)
        k += chunk
        assert_same_outputs(A, B, f"step_fused after {k}")
        assert_same_outputs(A, C, f"rollout_fused after {k}")
        window |= A.masks[..., T.atk_base(c):].ne(0).reshape(-1, c.R, c.R).any(0).cpu().numpy()
    if c.far:
        assert (window & ~T.disk(c, 1)).any(), f"no attack slot beyond one cell in any compared mask\n{window.astype(int)}"
    for e in (A, B, C):
        e.close()
    U, V, X = (mk(with_masks=False) for _ in range(3))
    for e in (U, V, X):
        e.reset()
    k = 0
    for chunk in (1, 19, 40):
        for i in range(chunk):
            U.uniform_policy(SEED, k + i)
            U.step(masks=False)
        V.rollout_uniform(SEED, k, chunk, fused=True)
        X.rollout_uniform(SEED, k, chunk, fused=False)
        k += chunk
        for e, form in ((V, "fused"), (X, "split")):
            U.synchronize()
            e.synchronize()
            for name in ("obs", "actions", "reward", "done"):
                same(getattr(e, name), getattr(U, name), name, f"rollout_uniform ({form}) after {k}")
            for s in range(0, n, 2):
                assert np.array_equal(U.dump_state(s), e.dump_state(s)), f"rollout_uniform ({form}) after {k}: state of slot {s}"
            assert not e.error_flags().any()
    for e in (U, V, X):
        e.close()


# ------------------------------------------------------------------ the uniform policy
@pytest.mark.parametrize("table", ["t5r3", "t8r5"])
def test_uniform_policy_matches_oracle(table):
    """mrts_policy_uniform_dev under a table: produce type in [0, nt), attack index in [0, R * R) — the oracle's
    restatement, 6 slots of 9x8, 5 steps."""
    c = T.TABLES[table]
    env = _env(table, 6, 0, [T.NOWHERE] * 6, seed=2)
    S, H, W, _, K = env.dims
    seen = np.zeros(7, np.int64)
    for step in (0, 1, 2, 7, 123456):
        env.uniform_policy(SEED, step)
        acts = env.actions.cpu().numpy().reshape(S, H * W, 7)
        for s in range(S):
            assert np.array_equal(acts[s], oracle_py.policy_uniform(H, W, K, SEED, s, step, c.nt)), f"slot {s} step {step}"
        seen = np.maximum(seen, acts.reshape(-1, 7).max(axis=0))
    assert seen.tolist() == [5, 3, 3, 3, 3, c.nt - 1, c.R * c.R - 1], f"largest component drawn {seen}"
    env.close()


# ------------------------------------------------------------------ observation encodings
OBS = [(t, shape) for t in ("t5r3", "t8r5") for shape in ("8x8", "16x16-po")]


@pytest.mark.parametrize("table,shape", OBS, ids=[f"{t}-{s}" for t, s in OBS])
def test_observation_encodings(table, shape):
    """onehot_obs, pack_obs / unpack_obs / onehot_packed and the records' renders (int32 and one-hot) with ntypes != 7,
    at steps 10, 30 and 60 of a masked rollout: the type field of the one-hot encoding is ntypes + 1 wide and moves
    every later channel.  Handle A steps one launch at a time; B runs the same rollout through the records.  The
    full-observability record holds 7 unit types at most and the one-hot render of records is for full observability
    only (both refusals asserted here), so the records are rendered for t5r3 (both forms) and t8r5 PO (int32)."""
    torch = torch_gpu()
    c = T.TABLES[table]
    po = shape.endswith("po")
    mp, n = (M16 if po else T.BASES8), 8
    kw = dict(partial_obs=True) if po else {}
    A = _env(table, n, 0, [mp] * n, seed=3, **kw)
    B = _env(table, n, 0, [mp] * n, seed=3, **kw)
    S, H, W, C, _ = A.dims
    F = 5 + 5 + 3 + (c.nt + 1) + 6 + 2 + (4 if po else 0)
    assert A._h.L.mrts_onehot_features(A._h.h) == F
    for e in (A, B):
        e.reset()
        e.random_policy(SEED, 0)
    assert B._h.L.mrts_exchange_init_loopback(B._h.h, 1, 0) == 0
    records = po or c.nt <= 7
    if records:
        words = B.set_records(64, 0)
    else:
        with pytest.raises(RuntimeError, match=r"-95.*<= 7 unit types"):
            B.set_records(64, 0)
    k, types = 0, set()
    for upto in (10, 30, 60):
        chunk = upto - k
        for i in range(chunk):
            A.step_fused(SEED, k + i + 1)
        if records:
            recv = B.records_buffer(chunk)
            off = B.rollout_fused_records(SEED, k + 1, chunk, recv)
        k = upto
        A.synchronize()
        B.synchronize()
        tag = f"step {k}"
        obs = A.obs.cpu().numpy()
        types |= set(np.unique(obs[:, 3]).tolist())
        want_hot = OR.onehot(obs, c.nt)
        assert want_hot.shape[-1] == F and np.array_equal(want_hot, encode_obs_np(obs, c.nt)), "the two numpy encodings differ"
        hot = A.onehot_obs()
        same(hot, want_hot, "one-hot observation", tag)
        buf = A.obs_packed_buffer(1, cap=H * W)
        A.pack_obs(buf[0])
        got = buf[0].cpu().view(torch.int32).numpy().view(np.uint32)
        assert np.array_equal(got, OR.pack(obs, H * W)), f"{tag}: packed rows"
        same(A.unpack_obs(buf).reshape(A.obs.shape), obs, "unpacked observation", tag)
        same(A.onehot_packed(buf).reshape(hot.shape), want_hot, "one-hot of the packed rows", tag)
        assert A.obs_pack_status() == (0, 0)
        if not records:
            continue
        # the records of the chunk's last step, rendered back: int32 planes and the one-hot batch of every slot
        o, stride = int(off[chunk - 1, 0]), int(off[chunk - 1, 1])
        assert stride % ((S // 2) * words) == 0
        out = torch.full(tuple(B.obs.shape), -7, dtype=torch.int32, device=B.device)
        B.render_records(recv, o, stride, 1, out)
        same(out, obs, "rendered records", tag)
        sel = torch.arange(S, dtype=torch.int32, device=B.device)
        if po:
            with pytest.raises(RuntimeError, match=r"-95.*full observability only"):
                B.render_records_onehot(recv, o, stride, sel)
        else:
            same(B.render_records_onehot(recv, o, stride, sel), want_hot, "one-hot of the records", tag)
        same(B.obs, obs, "obs of the records handle", tag)
        assert not B.render_overflow()
    assert (obs[:, 4] != 0).any(), "no unit action at step 60: nothing lies after the type field"
    if table == "t8r5" and not po:
        assert c.nt in types, f"no Tower (type plane {c.nt}) in any compared observation: {sorted(types)}"
    for e in (A, B):
        assert not e.error_flags().any()
        e.close()


# ------------------------------------------------------------------ forward model, checkpoint, state JSON, LightRush
@pytest.mark.parametrize("table", ["t8r5", "r5"])
def test_forward_model_matches_oracle(table):
    """ForwardModel(utt=table) against OracleForwardModel(utt_json=...) on melee8x8Mixed6: state dumps and float32
    evaluations (cost and hp come from the table) after every horizon."""
    torch_gpu()
    from microrts_amd import ForwardModel

    n = 16
    ai1, ai2, n1, n2 = fm_mixed(n)
    gpu = ForwardModel(n, T.MELEE8, policies=(n1, n2), utt=_utt(table), seed=21)
    ref = oracle_py.OracleForwardModel(n, T.MELEE8, ai1, ai2, seed=21, utt_json=T.utt_json(table))
    fm_compare(gpu, ref, n, "initial")
    seen = set()
    for chunk, horizon in enumerate([0, 1, 13, 50, 100]):
        gpu.playout(horizon)
        for g in range(n):
            ref.playout(g, horizon)
        fm_compare(gpu, ref, n, f"chunk {chunk} (horizon {horizon})")
        seen |= set(gpu.evaluate(0).cpu().numpy().tolist()) | set(gpu.evaluate(1).cpu().numpy().tolist())
    assert len(seen) >= 5, f"evaluation values seen: {sorted(seen)}"
    gpu.close()
    ref.close()


def test_checkpoint_restore_replays_identically():
    """Table r5 on 8x8: checkpoint, 40 steps, restore, the same 40 steps — observations, rewards, masks and states."""
    S = T.N_SP + T.N_BOT
    env = _env("r5", T.N_SP, T.N_BOT, [T.MELEE8] * S, ai2s=["RandomBiasedAI"] * T.N_BOT, seed=4)
    env.reset()
    for step in range(30):
        env.random_policy(9, step)
        env.step()
    ck = env.checkpoint()

    def run():
        out = []
        for step in range(30, 70):
            env.random_policy(9, step)
            env.step()
            env.synchronize()
            out.append([getattr(env, f).cpu().numpy().copy() for f in ("obs", "reward", "done", "masks", "actions")])
        return out, [env.dump_state(s) for s in range(S)]

    a, da = run()
    env.restore(ck)
    env.get_masks()
    b, db = run()
    for k, (x, y) in enumerate(zip(a, b)):
        for f, u, v in zip(("obs", "reward", "done", "masks", "actions"), x, y):
            assert np.array_equal(u, v), f"{f} differs at replayed step {k}"
    assert all(np.array_equal(x, y) for x, y in zip(da, db))
    assert any(not np.array_equal(x[0], a[0][0]) for x in a[1:]), "nothing moved in the replayed steps"
    assert not env.error_flags().any()
    env.close()


def test_state_json_round_trip():
    """get_state_json / set_state_json under table t8r5 (8 type names, a produced Tower): a mid-game state read as
    JSON and written into another game gives the same JSON and the same state dump up to unit positions in the
    list; the oracle, given the same text, holds the same state and the same masks."""
    n = 4
    env = _env("t8r5", n, 0, [T.BASES8] * n, seed=3)
    env.reset()
    for step in range(60):
        env.random_policy(SEED, step)
        env.step()
    text = env.state_json(0)
    st = json.loads(text)
    names = {u["type"] for u in st["pgs"]["units"]}
    assert st["actions"] and names <= set(_utt("t8r5").TYPES), f"types {names}, {len(st['actions'])} actions"
    env.set_state_json(2, text)
    assert env.state_json(2) == text
    assert np.array_equal(dumps.xy_free(env.dump_state(2)), dumps.xy_free(env.dump_state(0)))
    env.set_state_json(0, text)
    env.get_masks()
    env.synchronize()
    same(env.masks[2:4], env.masks[0:2].clone(), "masks of the copy", "after set_state_json")
    ref = oracle_py.OracleVecClient(n, 0, 2000, [T.BASES8] * n, seed=3, utt_json=T.utt_json("t8r5"))
    ref.reset()
    ref.set_state_json(0, text)
    assert np.array_equal(dumps.xy_free(env.dump_state(0)), dumps.xy_free(ref.dump(0))), "state against the oracle's"
    same(env.masks[0:2], ref.get_masks(0)[0:2], "masks", "after set_state_json, against the oracle")
    ref.close()
    assert not env.error_flags().any()
    env.close()


def test_lightrush_env_under_r5():
    """LightRush as the opponent of an agent under table r5 on 16x16, 200 steps of all-zero action rows (the CPU
    oracle has no LightRush).  Against the same environment under the built-in table, whose path the reference's
    traces pin: r5 differs from it in Ranged's range alone and LightRush trains Light units only, so no Ranged unit
    exists on basesWorkers16x16 (asserted) and the whole state, the observation, reward and done must agree at every
    step while the mask rows are 55 wide instead of 79.  And against the bot-only client under r5 with PassiveAI on
    the agent's side: time, resources, units and LightRush's assignments agree, as tests/test_gpu_lightrush_envs.py
    shows for the built-in table.  A table without a Light type is refused."""
    from microrts_amd import DeviceVecEnv, UnitTypeTable
    from tests.defs import RANGED

    agent = _env("r5", 0, 1, [M16], ai2s=["LightRush"], max_steps=5000)
    bots = _env("r5", 0, 1, [M16], ai1s=["PassiveAI"], ai2s=["LightRush"], max_steps=5000)
    builtin = DeviceVecEnv(0, 1, 5000, [M16], ai2s=["LightRush"])
    assert builtin.dims[4] == 79 and agent.dims[4] == 55
    for e in (agent, bots, builtin):
        e.players.zero_()
        e.reset()
    agent.actions.zero_()
    builtin.actions.zero_()
    busy = 0
    for k in range(201):
        da = agent.dump_state(0)
        assert np.array_equal(da, builtin.dump_state(0)), f"step {k}: state under r5 and under the built-in table"
        same(agent.obs, builtin.obs, "obs against the built-in table's", f"step {k}")
        same(agent.reward, builtin.reward, "reward against the built-in table's", f"step {k}")
        same(agent.done, builtin.done, "done against the built-in table's", f"step {k}")
        ta, ra, ua, aa = dumps.parse(da)
        assert not (ua[:, 0] == RANGED).any(), f"step {k}: a Ranged unit, the two tables may differ from here"
        tb, rb, ub, ab = dumps.parse(bots.dump_state(0))
        assert (ta, ra) == (tb, rb), f"step {k}: time / resources {(ta, ra)} vs {(tb, rb)}"
        assert np.array_equal(ua, ub), f"step {k}: units differ"
        mine_a, mine_b = aa[ua[aa[:, 0], 1] == 1], ab[ub[ab[:, 0], 1] == 1]
        assert np.array_equal(mine_a, mine_b), f"step {k}: LightRush's assignments differ\n{mine_a}\n{mine_b}"
        busy += len(mine_a)
        if k < 200:
            for e in (agent, bots, builtin):
                e.step()
    assert busy > 200, "LightRush hardly acted"
    for e in (agent, bots, builtin):
        assert not e.error_flags().any()
        e.close()
    no_light = UnitTypeTable.fromJSON(T.utt_json("r5").replace('"Light"', '"Lite"'))
    with pytest.raises(RuntimeError, match=r"-95.*type named Light"):
        DeviceVecEnv(0, 1, 2000, [M16], ai2s=["LightRush"], utt=no_light)
