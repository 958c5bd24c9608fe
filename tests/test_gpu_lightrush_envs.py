"""The native LightRush opponent in the environments around the pinned bot-only path
(tests/test_gpu_lightrush_traces.py): as the opponent of an agent, across checkpoints, beside other games of one
handle, and where it is refused."""
import os
import struct

import numpy as np
import pytest

from tests import dumps
from tests.gpu_support import torch_gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M8 = os.path.join(ROOT, "maps/8x8/basesWorkers8x8.xml")
M16 = os.path.join(ROOT, "maps/16x16/basesWorkers16x16.xml")


def _env(*a, **k):
    torch_gpu()
    from microrts_amd import DeviceVecEnv

    return DeviceVecEnv(*a, **k)


@pytest.mark.parametrize("side", [0, 1])
def test_agent_vs_lightrush_equals_the_bot_only_path(side):
    """JNIGridnetClient.gameStep with LightRush as ai2 (the agent plays `side`, all-zero action rows) against the
    bot-only client with PassiveAI on the agent's side — the path the reference traces pin.

    The agent's units hold NONE in both runs, of duration 1 under the zero rows (re-issued every step) and 10 under
    PassiveAI.  A NONE claims no cell and no resources, and LightRush reads of the other side only its units'
    positions, types and hit points: gs.free, gs.getResourceUsage and isUnitActionAllowed look at MOVE / PRODUCE
    assignments only, and getActionAssignment is asked for own units only.  So time, resources, the unit list and
    the LightRush side's assignments (type, parameter, issue time, in issue order) must agree at every step, and
    reward / done with them.  600 steps cross the first game's end (LightRush wins after about 480 steps) and the
    auto-reset: the second game must repeat the first, which it does only if the reset cleared the bot's memory."""
    steps = 600
    agent = _env(0, 1, 5000, [M8], ai2s=["LightRush"])
    bots = _env(0, 1, 5000, [M8], ai1s=["PassiveAI" if side == 0 else "LightRush"],
                ai2s=["LightRush" if side == 0 else "PassiveAI"])
    try:
        agent.players.fill_(side)
        # the bot-only client's `players` names the side ai1 plays (JNIBotClient.gameStep(player)): ai1 = player 0
        bots.players.zero_()
        agent.actions.zero_()
        agent.reset()
        bots.reset()
        lr = 1 - side
        history, ends = [], []
        for k in range(steps + 1):
            ta, ra, ua, aa = dumps.parse(agent.dump_state(0))
            tb, rb, ub, ab = dumps.parse(bots.dump_state(0))
            tag = f"step {k}"
            assert (ta, ra) == (tb, rb), f"{tag}: time / resources {(ta, ra)} vs {(tb, rb)}"
            assert np.array_equal(ua, ub), f"{tag}: units differ"
            mine_a = aa[ua[aa[:, 0], 1] == lr]
            mine_b = ab[ub[ab[:, 0], 1] == lr]
            assert np.array_equal(mine_a, mine_b), f"{tag}: LightRush's assignments differ\n{mine_a}\n{mine_b}"
            history.append((ta, ra, ua.copy(), mine_a.copy()))
            if k == steps:
                break
            agent.step()
            bots.step()
            da, db = int(agent.done.cpu()[0]), int(bots.done.cpu()[0])
            wa, wb = float(agent.reward.cpu()[0]), float(bots.reward.cpu()[0])
            # the agent's reward is its own side's, the bot-only client's is player 0's (ai1's): the same outcome
            assert da == db, f"{tag}: done {da} vs {db}"
            assert wa == (wb if side == 0 else -wb), f"{tag}: reward {wa} vs {wb}"
            if da:
                ends.append(k + 1)
        assert ends and ends[0] + 100 <= steps, f"no game over and 100 steps of a second game within {steps} steps: {ends}"
        n0 = ends[0]
        for j in range(steps - n0 + 1):  # the second game against the first
            t0, r0, u0, a0 = history[j]
            t1, r1, u1, a1 = history[n0 + j]
            assert (t0, r0) == (t1, r1) and np.array_equal(u0, u1) and np.array_equal(a0, a1), \
                f"step {j} of the second game differs from the first game's"
        assert not agent.error_flags().any() and not bots.error_flags().any()
    finally:
        agent.close()
        bots.close()


def _bot_memory(ckpt, game=0):
    """The LightRush memory of one game out of checkpoint bytes (mrts_internal.h: the words after stateWords in
    each block, per player a 4-word header and the arrays ACT, REF, RANK of CAP words): -> (units in use,
    [player][slot] action kinds)."""
    magic, version, H, W, cap, n_games, n_sp, words = struct.unpack_from("<8s7i", ckpt, 0)
    assert magic == b"MRTSCKP1"
    blocks = np.frombuffer(ckpt, dtype=np.int32, offset=48).reshape(n_games, words)
    per_player = 4 + 3 * cap
    mem = blocks[game, words - 2 * per_player:].reshape(2, per_player)
    return int(blocks[game, 1]), (mem[:, 4:4 + cap] & 7)


def _bot_words(ckpt, game=0):
    """every word of one game's LightRush memory in checkpoint bytes"""
    _, _, _, _, cap, n_games, _, words = struct.unpack_from("<8s7i", ckpt, 0)
    return np.frombuffer(ckpt, dtype=np.int32, offset=48).reshape(n_games, words)[game, words - 2 * (4 + 3 * cap):]


def test_checkpoint_carries_the_bot_memory():
    """LightRush against itself on 16x16: a checkpoint taken mid-build (step 137: a worker holds a Build or a
    Harvest) and restored must replay the same 200 steps — which needs the abstract actions, their insertion
    order and Train's completed flags, not only the game state."""
    env = _env(0, 1, 5000, [M16], ai1s=["LightRush"], ai2s=["LightRush"])
    try:
        env.reset()
        for _ in range(137):
            env.step()
        ck = env.checkpoint()
        nu, kinds = _bot_memory(ck)
        held = kinds[:, :nu]
        assert ((held == 2) | (held == 3)).any(), f"no Build / Harvest held at step 137: {held.tolist()}"
        first = []
        for _ in range(200):
            env.step()
            first.append(env.dump_state(0))
        assert any(not np.array_equal(first[0], d) for d in first[1:])
        ck_end = env.checkpoint()
        env.restore(ck)
        for k in range(200):
            env.step()
            d = env.dump_state(0)
            assert np.array_equal(d, first[k]), f"step {137 + k + 1} after the restore differs"
        # the memory's bytes are a function of the games played (units born and removed in these 200 steps included:
        # nothing but written words reaches the state block)
        assert np.array_equal(_bot_words(ck_end), _bot_words(env.checkpoint())), "bot memory bytes differ after the same steps"
        # the same state without the memory is another game: the bots start over (a restored memory matters)
        env.restore(ck)
        env.set_state_json(0, env.state_json(0))
        nu2, kinds2 = _bot_memory(env.checkpoint())
        assert nu2 == nu and not kinds2.any(), "mrts_set_state_json left bot memory behind"
        assert not env.error_flags().any()
    finally:
        env.close()


def test_lightrush_game_leaves_the_other_games_of_its_handle_alone():
    """Two self-play slots, a RandomBiasedAI environment and a LightRush environment in one handle, 100 steps of
    unmasked uniform actions: observations, masks, rewards, done flags and states of the first three slots equal
    those of the same handle built without the LightRush environment (whose state blocks are shorter)."""
    import torch

    steps = 100
    maps = [M8] * 4
    a = _env(2, 2, 2000, maps, ai2s=["RandomBiasedAI", "LightRush"], seed=5)
    b = _env(2, 1, 2000, maps[:3], ai2s=["RandomBiasedAI"], seed=5)
    try:
        S, H, W, C, K = b.dims
        # 8x8: CAP = 128, stateWords = 996; only the handle with the LightRush game carries botWords(128) = 776
        # (two self-play slots are one game: 2 and 3 games)
        assert len(b.checkpoint()) == 48 + 2 * 996 * 4 and len(a.checkpoint()) == 48 + 3 * (996 + 776) * 4
        a.reset()
        b.reset()
        rng = np.random.default_rng(11)
        HW = H * W
        for k in range(steps):
            acts = np.stack([rng.integers(0, 6, (4, HW)), rng.integers(0, 4, (4, HW)), rng.integers(0, 4, (4, HW)),
                             rng.integers(0, 4, (4, HW)), rng.integers(0, 4, (4, HW)), rng.integers(0, 7, (4, HW)),
                             rng.integers(0, K - 23 - 7, (4, HW))], axis=-1).astype(np.int32)
            a.actions.copy_(torch.as_tensor(acts))
            b.actions.copy_(torch.as_tensor(acts[:3]))
            a.step()
            b.step()
            tag = f"step {k}"
            assert torch.equal(a.obs[:3], b.obs), f"{tag}: observations"
            assert torch.equal(a.masks[:3], b.masks), f"{tag}: masks"
            assert torch.equal(a.reward[:3], b.reward) and torch.equal(a.done[:3], b.done), f"{tag}: reward / done"
            if k % 10 == 9:
                for s in range(3):
                    assert np.array_equal(a.dump_state(s), b.dump_state(s)), f"{tag}: state of slot {s}"
        t, _, units, asg = dumps.parse(a.dump_state(3))
        assert t == steps and len(asg) > 0  # the LightRush environment ran beside them
        assert not a.error_flags().any() and not b.error_flags().any()
    finally:
        a.close()
        b.close()


def test_evaluate_and_copy_read_the_longer_blocks():
    """mrts_evaluate ("of every game") and mrts_copy_games' source side on a handle whose state blocks carry the bot
    memory: three different games (LightRush against LightRush, PassiveAI, RandomBiasedAI) after 400 steps are
    evaluated in place and, copied into a ForwardModel (blocks without bot memory), evaluated there — the same
    values, game by game, and the copies' states equal the originals'."""
    import ctypes

    from microrts_amd import ForwardModel

    n = 3
    env = _env(0, n, 5000, [M8] * n, ai1s=["LightRush"] * n, ai2s=["LightRush", "PassiveAI", "RandomBiasedAI"], seed=3)
    fm = ForwardModel(n, M8, policies=("PassiveAI", "PassiveAI"))
    try:
        env.reset()
        for _ in range(400):  # (at 150 steps the first two games are still mirror-symmetric: both evaluate to 0)
            env.step()
        env.synchronize()
        fm.copy_from([[g, g] for g in range(n)], src=env)
        for g in range(n):
            a, b = dumps.parse(env.dump_state(g)), dumps.parse(fm.dump_state(g))
            assert a[:2] == b[:2] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), f"copy of game {g}"
        seen = []
        for maxplayer in (0, 1):
            here = np.zeros(n, np.float32)
            h = env._h
            rc = h.L.mrts_evaluate(h.h, maxplayer, here.ctypes.data_as(ctypes.c_void_p))
            assert rc == 0, h.L.mrts_last_error().decode()
            there = fm.evaluate(maxplayer).cpu().numpy()
            assert np.array_equal(here, there), f"maxplayer {maxplayer}: {here} on the handle, {there} on the copies"
            seen.append(here)
        assert len(set(seen[0].tolist())) == n, f"the three games evaluate alike ({seen[0]}): the comparison shows nothing"
    finally:
        fm.close()
        env.close()


def test_refusals():
    """What the native LightRush does not do is refused with -ENOTSUP (errno 95) and a message naming the reason."""
    from microrts_amd import DeviceVecEnv, ForwardModel, UnitTypeTable
    from microrts_amd.vec_client import _bot_kind

    with pytest.raises(RuntimeError, match=r"-95.*partial_obs \+ LightRush"):
        DeviceVecEnv(0, 1, 2000, [M8], ai2s=["LightRush"], partial_obs=True)
    with pytest.raises(RuntimeError, match=r"-95.*forward-model playout policy"):
        ForwardModel(1, M8, policies=("LightRush", "RandomBiasedAI"))
    with pytest.raises(RuntimeError, match=r"-95.*forward-model playout policy"):
        ForwardModel(1, M8, policies=("PassiveAI", "LightRush"))
    no_light = UnitTypeTable.fromJSON(UnitTypeTable().toJSON().replace('"Light"', '"Lite"'))
    assert "Lite" in no_light.TYPES and "Light" not in no_light.TYPES
    with pytest.raises(RuntimeError, match=r"-95.*type named Light"):
        DeviceVecEnv(0, 1, 2000, [M8], ai2s=["LightRush"], utt=no_light)
    big = os.path.join(ROOT, "maps/BroodWar/(3)Aztec.scxA.xml")
    with pytest.raises(RuntimeError, match=r"-95.*more than 1024 cells"):  # a 128x128 map
        DeviceVecEnv(0, 1, 2000, [big], ai1s=["LightRush"], ai2s=["LightRush"], max_units=1024)
    # the bot-only client plays on the full state whatever partial_obs says (JNIBotClient has no view): accepted
    e = DeviceVecEnv(0, 1, 2000, [M8], ai1s=["LightRush"], ai2s=["LightRush"], partial_obs=True)
    e.close()
    with pytest.raises(NotImplementedError):
        _bot_kind("WorkerRush")
