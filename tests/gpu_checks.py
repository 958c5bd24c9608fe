"""Check bodies that more than one test file runs on its own scenarios (a plain helper module: every assert carries
its own message).  tests/test_gpu_parity.py, test_headline_parity.py, test_forward_model.py and
test_full_size_every_game.py call them on the standard maps, tests/test_gpu_combat.py on combat maps,
tests/test_gpu_issue_both.py and tests/test_gpu_ablate.py run flag_rollout / doubled_rollout in a child process and
tools/soak_long.py runs every_game over longer horizons."""
import concurrent.futures as cf

import numpy as np

from tests import oracle_py
from tests.defs import SEED
from tests.gpu_support import assert_matches_oracle, same, torch_gpu

RB, PASSIVE = oracle_py.BOT_RANDOM_BIASED, oracle_py.BOT_PASSIVE
FUSED_MAP = "maps/16x16/basesWorkers16x16.xml"


def oracle_threads():
    """The CPUs this process may use, capped by the cgroup quota (16 on the GPU box)."""
    import bench

    return min(16, bench.all_cores())


def rollout(maps, n_sp, n_bot=0, steps=200, max_steps=2000, utt=1, crs=1, policy="masked", dump_every=10, seed=3,
            players=None, partial_obs=False, bots=None, rfs=None, utt_json=None, max_units=0, reach=None):
    """One launch per step against the oracle, the same int32 action rows on both sides: masks before every step,
    the policy kernel's rows (masked policy), observations, rewards and dones after it, every slot's state dump
    every dump_every steps.  -> the handle's error flags; rollout.nonzero (set by the caller, one bool per reward
    function) collects which reward functions fired; reach (tests.table_cases.Reach) is shown the oracle's masks of every step."""
    torch = torch_gpu()
    from microrts_amd import DeviceVecEnv, UnitTypeTable

    table = UnitTypeTable.fromJSON(utt_json) if utt_json else UnitTypeTable(utt, crs)
    ntypes = len(table.TYPES)
    env = DeviceVecEnv(n_sp, n_bot, max_steps, maps, utt=table, seed=seed, partial_obs=partial_obs,
                       ai2s=bots, rfs=rfs, max_units=max_units)
    kinds = [1 if b == "RandomBiasedAI" else 0 for b in bots] if bots else None
    ref = oracle_py.OracleVecClient(n_sp, n_bot, max_steps, maps, utt_version=utt, crs=crs, seed=seed,
                                    partial_obs=partial_obs, bot_kinds=kinds,
                                    rewards=[oracle_py.REWARD_IDS[r] for r in rfs] if rfs else None, utt_json=utt_json)
    S = ref.S
    if players is not None:
        env.players.copy_(torch.as_tensor(players, dtype=torch.int32))
    env.reset()
    ref.reset(players)
    assert_matches_oracle(env, ref, "reset", masks=None)
    rng = np.random.default_rng(seed)
    HW = ref.H * ref.W
    for step in range(steps):
        m_ref = ref.get_masks(0)
        env.synchronize()
        same(env.masks, m_ref, "masks", f"step {step}")
        if reach is not None:
            reach.add(m_ref)
        if policy == "masked":
            env.random_policy(SEED, step)
            env.synchronize()
            acts = env.actions.cpu().numpy()
            if step < 20 or step % 10 == 0:  # the GPU policy kernel is bit-identical to the oracle's Philox policy
                for s in range(min(S, 8)):
                    assert np.array_equal(acts[s], oracle_py.policy(m_ref[s], SEED, s, step, 0, ntypes)), \
                        f"step {step}: policy rows of slot {s}"
        else:  # unmasked uniform components (exercises every illegal → NONE path)
            acts = np.stack([rng.integers(0, 6, (S, HW)), rng.integers(0, 4, (S, HW)), rng.integers(0, 4, (S, HW)),
                             rng.integers(0, 4, (S, HW)), rng.integers(0, 4, (S, HW)), rng.integers(0, ntypes, (S, HW)),
                             rng.integers(0, ref.K - 23 - ntypes, (S, HW))], axis=-1).astype(np.int32)
            env.actions.copy_(torch.as_tensor(acts))
        env.step()
        ref.step(acts, players)
        assert_matches_oracle(env, ref, f"step {step + 1}", masks=None,
                              states="all" if dump_every and (step + 1) % dump_every == 0 else None)
        if rfs:
            rollout.nonzero |= (ref.reward != 0).reshape(ref.S, -1).any(axis=0)
    flags = env.error_flags()
    env.close()
    ref.close()
    return flags


def encode_obs_np(obs, ntypes):
    """numpy restatement of MicroRTS-Py's GridnetVecEnv `_encode_obs` (gym_microrts, external to the
    reference — parity unpinned): per env, planes clipped to [0, n-1] and one-hot encoded, channels
    last, plane sizes [5, 5, 3, ntypes + 1, 6, 2] (+ [2] per extra partial-observability plane)."""
    S, C, H, W = obs.shape
    sizes = [5, 5, 3, ntypes + 1, 6, 2] + [2] * (C - 6)
    offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    out = np.zeros((S, H * W, sum(sizes)), np.uint8)
    flat = obs.reshape(S, C, H * W)
    for p in range(C):
        v = np.clip(flat[:, p], 0, sizes[p] - 1)
        np.put_along_axis(out, (v + offs[p])[..., None], 1, axis=2)
    return out.reshape(S, H, W, -1)


def onehot_encoder(mp, po):
    """mrts_onehot_dev = MicroRTS-Py's observation encoding of the step's int32 observation."""
    torch_gpu()
    from microrts_amd import DeviceVecEnv

    env = DeviceVecEnv(6, 0, 2000, [mp] * 6, seed=3, partial_obs=po)
    env.reset()
    for step in range(60):
        env.random_policy(SEED, step)
        env.step()
        if step % 10 == 9:
            got = env.onehot_obs()
            env.synchronize()
            ref = encode_obs_np(env.obs.cpu().numpy(), 7)
            assert got.shape[-1] == (33 if po else 29), f"step {step}: {got.shape[-1]} one-hot channels"
            same(got, ref, "one-hot observation", f"step {step}")
    env.close()


def fm_mixed(n):
    """Playout policies of n forward-model games, as oracle kinds and as names: (ai1, ai2, names1, names2)."""
    ai1 = [RB, RB, PASSIVE, RB] * (n // 4)
    ai2 = [RB, PASSIVE, RB, RB] * (n // 4)
    name = {RB: "RandomBiasedAI", PASSIVE: "PassiveAI"}
    return ai1, ai2, [name[k] for k in ai1], [name[k] for k in ai2]


def fm_compare(gpu, ref, n, tag, evals=True):
    """The HIP forward model's n games against the oracle's: state dumps, float32 evaluations, no error flag."""
    for g in range(n):
        assert np.array_equal(gpu.dump_state(g), ref.dump(g)), f"{tag}: state of game {g}"
    if evals:
        for mp in (0, 1):
            v = gpu.evaluate(mp).cpu().numpy()
            for g in range(n):
                assert v[g] == ref.evaluate(g, mp), \
                    f"{tag}: evaluation of game {g} for player {mp}: gpu {v[g]} ref {ref.evaluate(g, mp)}"
    assert not gpu.error_flags().any(), f"{tag}: error flags {gpu.error_flags()}"


# flag_rollout's shapes: map, launches (steps each), partially observable, max_units, uniform policy without masks
FLAG_ROLLOUTS = {"16x16 fused": (FUSED_MAP, (1, 19, 80, 100), False, 0, False),
                 "8x8 uniform": ("maps/8x8/basesWorkers8x8.xml", (1, 19, 40), False, 0, True),
                 "32x32 PO fused": ("maps/BWDistantResources32x32.xml", (1, 19, 40), True, 256, False)}


def flag_rollout(out, shape="16x16 fused", before=None):
    """A rollout of 32 slots (by default the 16x16 fused one of 200 steps); everything it leaves, to `out` (.npz).
    before: called once the library is loaded, ahead of the first launch (a diagnostic build's switches)"""
    torch_gpu()
    from microrts_amd import DeviceVecEnv

    S = 32
    mp, launches, po, mu, uniform = FLAG_ROLLOUTS[shape]
    env = DeviceVecEnv(S, 0, 2000, [mp] * S, seed=9, partial_obs=po, max_units=mu, with_masks=not uniform)
    if before:
        before()
    env.reset()
    if not uniform:
        env.random_policy(SEED, 0)
    res, k = {}, 0
    for n in launches:
        if uniform:
            env.rollout_uniform(SEED, k, n)
        else:
            env.rollout_fused(SEED, k + 1, n)
        k += n
        env.synchronize()
        for name in ("obs", "actions", "reward", "done") if uniform else ("obs", "masks", "actions", "reward", "done"):
            res[f"{name}_{k}"] = getattr(env, name).cpu().numpy()
        for s in range(0, S, 2):
            res[f"state_{k}_{s}"] = env.dump_state(s)
    res["flags"] = env.error_flags()
    env.close()
    np.savez(out, **res)


def doubled_rollout(out, shape):
    """tests/test_gpu_ablate.py's child, whose library is the ablation build: flag_rollout with every row of kind AGAIN
    of the library's own table (mrts_ablate_phase) set — each runs its phase of the step a second time — and the
    COUNT row, whose render counters show on the partially observable shape that the word reached the kernels"""
    import ctypes

    from microrts_amd import _lib
    from tools import ablate_table

    L, phases = ablate_table.load(_lib.LIB_PATH)

    def every_doubling():
        again = [p for p in phases if p.kind == "AGAIN"]
        assert len(again) >= 20, again  # (a table that lost its rows cannot pass)
        assert L.mrts_set_ablate(ablate_table.mask(again + [p for p in phases if p.kind == "COUNT"])) == 0

    flag_rollout(out, shape, before=every_doubling)
    if FLAG_ROLLOUTS[shape][2]:
        dbg = (ctypes.c_ulonglong * 4)()
        assert L.mrts_get_dbg(dbg, 0) == 0 and dbg[1] > 0, f"no render counted: {list(dbg)}"


def record_exchange_loopback_ranks(mp, po, spl, world, rank):
    """The records exchange's multi-rank layout on one GPU (tests/test_headline_parity.py
    test_record_exchange_loopback_ranks tells what is checked and why)."""
    torch = torch_gpu()
    from microrts_amd import DeviceVecEnv

    n_sp = 64
    kw = dict(partial_obs=True, max_units=256) if po else {}
    A = DeviceVecEnv(n_sp, 0, 300, [mp] * n_sp, seed=29, **kw)
    B = DeviceVecEnv(n_sp, 0, 300, [mp] * n_sp, seed=29, **kw)
    C = DeviceVecEnv(n_sp, 0, 300, [mp] * n_sp, seed=29, **kw)  # B's twin, never in the steady state at a call
    A.set_multi_step(False)
    for e in (A, B, C):
        e.reset()
        e.random_policy(SEED, 0)
    L, h = B._h.L, B._h.h
    assert L.mrts_exchange_init_loopback(h, world, world) != 0, "a rank out of range was accepted"
    assert L.mrts_exchange_init_loopback(h, world, rank) == 0, "mrts_exchange_init_loopback failed"
    assert L.mrts_exchange_init_loopback(h, world, rank) != 0, "a second mrts_exchange_init_loopback was accepted"
    assert L.mrts_exchange_init_loopback(C._h.h, world, rank) == 0, "mrts_exchange_init_loopback failed on the twin"
    words = B.set_records(64, spl)
    assert C.set_records(64, spl) == words, "the twin's record size differs"
    distinct = 0  # steps whose games differed, so that a wrong rank place would have shown
    G = n_sp // 2
    k = 0
    for n in (1, 40, 25):
        want = []
        for j in range(n):
            A.rollout_fused(SEED, k + j + 1, 1)
            A.synchronize()
            want.append(A.obs.clone())
        recv = B.records_buffer(n, world)
        recv.fill_(-7)  # every record header the exchange owes must be written (unit words past n are don't-care)
        off = B.rollout_fused_records(SEED, k + 1, n, recv)
        C.get_masks()  # C leaves the steady fused state: its first launch of the call runs one step alone
        recvC = C.records_buffer(n, world)
        recvC.fill_(-7)  # (as recv: unit words past a record's n stay as they were)
        offC = C.rollout_fused_records(SEED, k + 1, n, recvC)
        assert np.array_equal(off, offC), "the chunk schedule must not depend on the steady state"
        k += n
        B.synchronize()
        C.synchronize()
        same(recv, recvC, "receive buffer of the unsteady twin", f"after {k}")
        for j in range(n):
            at = f"step {k - n + j}"
            o, stride = int(off[j, 0]), int(off[j, 1])
            assert stride >= G * words and (o + (world - 1) * stride + G * words) <= recv.numel(), \
                f"{at}: offset {o} / stride {stride} outside the receive buffer of {recv.numel()} words"
            mine = recv[o + rank * stride:o + rank * stride + G * words]
            assert not bool((mine.view(G, words)[:, 0] == -7).any()), f"{at}: a record header never written"
            for r in range(world):  # peer r: this rank's game (g + r - rank) mod G at its game g
                peer = recv[o + r * stride:o + r * stride + G * words].view(G, words)
                same(peer, torch.roll(mine.view(G, words), -(r - rank), 0), f"records of rank {r}", at)
            out = torch.zeros((world * 2 * G,) + tuple(B.obs.shape[1:]), dtype=torch.int32, device=B.device)
            B.render_records(recv, o, stride, world, out)
            B.synchronize()
            for r in range(world):
                same(out[r * 2 * G:(r + 1) * 2 * G], torch.roll(want[j], -2 * (r - rank), 0), f"rendered rank {r}", at)
            # the check can fail: once the games differ, the neighbour's place rendered as this rank's is not
            # this rank's observation (right after a reset every game may still look the same)
            if not torch.equal(torch.roll(want[j], -2, 0), want[j]):
                nb = (rank + 1) % world
                wrong = torch.zeros_like(B.obs)
                B.render_records(recv, o + nb * stride, stride, 1, wrong)
                B.synchronize()
                assert not torch.equal(wrong, want[j]), f"{at}: a neighbour's place renders like this rank's"
                distinct += 1
        same(B.obs, A.obs, "obs", f"after {k}")
        same(B.masks, A.masks, "masks", f"after {k}")
    if not po:  # the per-step tensor exchange: [ranks][slots][C][H][W]
        send = [torch.zeros(tuple(B.obs.shape), dtype=torch.int16, device=B.device) for _ in range(2)]
        tr = torch.full((world,) + tuple(B.obs.shape), -7, dtype=torch.int16, device=B.device)
        A.rollout_fused(SEED, k + 1, 3)
        B.rollout_fused_exchange(SEED, k + 1, 3, send, tr)
        A.synchronize()
        B.synchronize()
        for r in range(world):  # peer r: this rank's slot (i + r - rank) mod slots at its slot i
            same(tr[r], torch.roll(A.obs.to(torch.int16), -(r - rank), 0), f"tensor exchange rank {r}", f"after {k + 3}")
    assert distinct > 10, "the games never differed: the rank checks could not fail"
    for name, e in zip("ABC", (A, B, C)):
        assert not e.error_flags().any(), f"error flags of {name}: {e.error_flags()}"
        e.close()


# ------------------------------------------------------------------ every game of a benchmark configuration
POINTS = (1000, 20, 200)  # burn-in, then the driver's K and the bench default, as single rollout calls
# config: map, games, partially observable, max_units, seed, uniform policy
SHAPES = {"c3": ("maps/16x16/basesWorkers16x16.xml", 4096, False, 0, 5, False),
          "c5": ("maps/BWDistantResources32x32.xml", 2048, True, 256, 7, False),
          "c2": ("maps/8x8/basesWorkers8x8.xml", 1024, False, 0, 8, True)}


def _gpu_points(cfg):
    """The GPU rollout in the bench's form; a host snapshot of every output and every state at each point."""
    torch_gpu()
    from microrts_amd import DeviceVecEnv

    mp, E, po, mu, seed, uniform = SHAPES[cfg]
    S = 2 * E
    env = DeviceVecEnv(S, 0, 2000, [mp] * S, seed=seed, partial_obs=po, max_units=mu, with_masks=not uniform)
    assert env.multi_step_capable if uniform else env.fused_multi_step, "the bench's shape must run multi-step launches"
    env.reset()
    if not uniform:
        env.random_policy(SEED, 0)
    snaps, t = [], 0
    for n in POINTS:
        if uniform:
            env.rollout_uniform(SEED, t, n, fused=True)
        else:
            env.rollout_fused(SEED, t + 1, n)  # the first launch is a single step, then multi-step launches
        t += n
        env.synchronize()
        snap = {k: getattr(env, k).cpu().numpy() for k in ("obs", "reward", "done", "actions")}
        if not uniform:
            snap["masks"] = env.masks.cpu().numpy()
        snap["state"] = [env._h.dump(s) for s in range(S)]
        snaps.append((t, snap))
    assert not env.error_flags().any(), f"{cfg}: error flags {env.error_flags()}"
    env.close()
    return snaps


def _shard(cfg, g0, g1, snaps):
    """Oracle replicas of games [g0, g1): run to each point, compare; -> {what: mismatching slots}, examples."""
    mp, E, po, mu, seed, uniform = SHAPES[cfg]
    slots = np.arange(2 * g0, 2 * g1)
    ref = oracle_py.OracleVecClient(len(slots), 0, 2000, [mp] * len(slots), seed=seed, partial_obs=po)
    ref.reset()
    H, W, K = ref.H, ref.W, ref.K
    bad, ex, t = {}, [], 0
    for t_end, snap in snaps:
        ref.rollout_policy(t_end - t, SEED, 2 * g0, t, uniform=uniform)
        t = t_end
        got = {"obs": ref.obs, "reward": ref.reward, "done": ref.done}
        if uniform:  # the tensor holds the rows of the launch's last step
            got["actions"] = np.stack([oracle_py.policy_uniform(H, W, K, SEED, int(s), t - 1) for s in slots])
        else:  # the masks of the last step and the rows the launch sampled from them for the next step
            m = ref.get_masks(0)
            got["masks"] = m
            got["actions"] = np.stack([oracle_py.policy(m[i], SEED, int(s), t, 0) for i, s in enumerate(slots)])
        for f, want in got.items():
            g = np.asarray(snap[f][2 * g0:2 * g1]).reshape(len(slots), -1)
            ok = (g == np.asarray(want).reshape(len(slots), -1)).all(axis=1)
            if not ok.all():
                bad[f"step {t}: {f}"] = int((~ok).sum())
                ex.append((t, f, [int(s) for s in slots[~ok][:4]]))
        nst = [int(s) for i, s in enumerate(slots) if not np.array_equal(snap["state"][s], ref.dump(i))]
        if nst:
            bad[f"step {t}: state"] = len(nst)
            ex.append((t, "state", nst[:4]))
    ref.close()
    return bad, ex


def every_game(cfg):
    """Every game of a benchmark configuration against oracle replicas, at each of POINTS (tests/test_full_size_every_game.py)."""
    snaps = _gpu_points(cfg)
    E = SHAPES[cfg][1]
    nt = oracle_threads()
    step = (E + nt - 1) // nt
    bad, ex = {}, []
    with cf.ThreadPoolExecutor(nt) as pool:  # the oracle steps in native code with the GIL released
        for b, e in pool.map(lambda g0: _shard(cfg, g0, min(g0 + step, E), snaps), range(0, E, step)):
            for k, v in b.items():
                bad[k] = bad.get(k, 0) + v
            ex += e
    assert not bad, f"{cfg}: mismatching slots {bad}; first cases (step, field, slots) {ex[:8]}"
