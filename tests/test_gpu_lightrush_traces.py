"""The native LightRush opponent against the reference's own LightRush games.

src/tests/GenerateTestTraces.java:84-123 produced the `LightRush_AStarPathFinding_` traces by running
LightRush(UTT) against a clone of itself from the map: ai1.getAction(0, gs), ai2.getAction(1, gs), issueSafe(pa1),
issueSafe(pa2), cycle() — the loop of JNIBotClient.gameStep(0) (src/tests/JNIBotClient.java:108-135), which the
bot-only client runs on the GPU.  So a bot-only environment with LightRush on both sides, started from the map,
must pass through every PhysicalGameState the trace recorded: after k steps the game's clock is k, and before the
step at an entry's time the state dump must equal that entry (time, both players' resources, every unit in list
order).  Nothing of ours sits in between: no oracle, no recorded actions.

A trace that ends by game over before cycle 500 (MAX_CYCLES) must raise `done` on exactly the step that reaches its
last entry's time, with the WinLoss reward of the side that entry shows alive; the final state itself is gone after
the auto-reset.  A trace that runs to 500 has its last entry compared like the others.

Every map of at most 1024 cells (the native A*'s limit) is covered: 94 traces.  EXCLUDED is the list of traces the
present reference source provably does not reproduce; it is empty.
"""
import gzip
import os

import numpy as np
import pytest

from tests.gpu_support import torch_gpu
from tests.trace_fixtures import GROUPS, IDX, ROOT, SIZES, TR, check_vs_trace, parse

pytestmark = pytest.mark.gpu

LIMIT = 1024  # H * W of the largest map the native LightRush plays (mrts_internal.h LR_MAX_CELLS)
STEPS = 500   # GenerateTestTraces.MAX_CYCLES
EXCLUDED = ()  # fixture names; at most 3, each with a hand derivation in this docstring — none is needed


def _lr(group):
    return [e for e in group if e["fixture"].endswith("__LightRush.trace.gz") and e["fixture"] not in EXCLUDED]


LR_SIZES = [s for s in SIZES if s[0] * s[1] <= LIMIT and _lr(GROUPS[s])]


def _entries(e):
    ent = parse(gzip.open(os.path.join(TR, e["fixture"]), "rt").read())
    assert len(ent) == e["entries"]
    return ent


def _survivor_reward(units):
    """WinLossRewardFunction for player 0 of a finished game whose last state holds `units`: winner() == 0 ? 1 : -1
    (src/ai/reward/WinLossRewardFunction.java:16-24) — a game that both sides lose in the same cycle
    (basesWorkersBarracks8x8: only the resources are left) has winner -1, so -1 as well."""
    alive = {int(p) for p in units[:, 1] if p >= 0}
    assert len(alive) <= 1, "the trace's last entry is no game over"
    return 1.0 if alive == {0} else -1.0


def _run(group, ai1, ai2, stop_at_mismatch=False):
    """Play the group's maps bot against bot and compare with the traces.  Returns the number of entries compared
    (or, with stop_at_mismatch, the (game, entry index) of the first entry that differs, None if none does)."""
    torch_gpu()
    from microrts_amd import DeviceVecEnv

    n = len(group)
    traces = [_entries(e) for e in group]
    at = [{} for _ in range(n)]  # per game: time -> entry indices
    for g, ent in enumerate(traces):
        for k, en in enumerate(ent):
            at[g].setdefault(en[0], []).append(k)
    last = [ent[-1][0] for ent in traces]
    env = DeviceVecEnv(0, n, 2000, [os.path.join(ROOT, e["map"]) for e in group], ai1s=[ai1] * n, ai2s=[ai2] * n)
    compared = 0
    try:
        env.players.zero_()
        env.reset()
        over = [False] * n
        for k in range(STEPS + 1):
            for g in range(n):
                if over[g] or k not in at[g]:
                    continue
                if last[g] < STEPS and k == last[g]:
                    continue  # the state a game over left: replaced by the auto-reset (checked through done below)
                d = env.dump_state(g)
                for i in at[g][k]:
                    try:
                        check_vs_trace(d, traces[g][i], f"{group[g]['map']} entry {i} (time {k})")
                    except AssertionError:
                        if stop_at_mismatch:
                            return g, i
                        raise
                    compared += 1
            if k == STEPS:
                break
            env.step()
            done = env.done.cpu().numpy().reshape(n, -1)[:, 0]
            rew = env.reward.cpu().numpy().reshape(n, -1)[:, 0]
            for g in range(n):
                if over[g]:
                    continue
                ends = last[g] < STEPS and k + 1 == last[g]
                if stop_at_mismatch and bool(done[g]) != ends:
                    return g, len(traces[g]) - 1
                assert bool(done[g]) == ends, f"{group[g]['map']}: done = {done[g]} after step {k} (the trace ends at {last[g]})"
                if ends:
                    want = _survivor_reward(traces[g][-1][2])
                    assert rew[g] == want, f"{group[g]['map']}: WinLoss reward {rew[g]} vs {want} at the trace's end"
                    over[g] = True
                    compared += 1
        assert not env.error_flags().any()
    finally:
        env.close()
    return None if stop_at_mismatch else compared


@pytest.mark.parametrize("size", LR_SIZES, ids=[f"{h}x{w}" for h, w in LR_SIZES])
def test_lightrush_reproduces_the_reference_traces(size):
    group = _lr(GROUPS[size])
    n = _run(group, "LightRush", "LightRush")
    assert n == sum(e["entries"] for e in group)


def test_every_lightrush_trace_up_to_the_limit_is_covered():
    """94 LightRush fixtures on maps of at most 32x32, by size; none skipped beyond EXCLUDED's cap."""
    want = {(4, 4): 7, (8, 8): 25, (8, 9): 1, (8, 16): 1, (10, 10): 1, (12, 12): 20, (12, 14): 1, (12, 16): 1, (14, 15): 1,
            (16, 16): 18, (24, 24): 15, (32, 32): 3}
    all_lr = {s: [e for e in GROUPS[s] if e["fixture"].endswith("__LightRush.trace.gz")] for s in SIZES}
    assert {s: len(v) for s, v in all_lr.items() if s[0] * s[1] <= LIMIT} == want
    assert sum(want.values()) == 94 and sum(len(v) for v in all_lr.values()) == 140
    assert sorted(LR_SIZES) == sorted(want)
    assert sum(len(_lr(GROUPS[s])) for s in LR_SIZES) == 94 - len(EXCLUDED)
    assert len(EXCLUDED) <= 3
    for name in EXCLUDED:
        assert not any(k in name for k in ("basesWorkers8x8__", "basesWorkers16x16__", "BWDistantResources32x32"))
        assert any(e["fixture"] == name for e in IDX)


def test_a_different_opponent_does_not_match_the_trace():
    """The comparison is not vacuous: basesWorkers8x8 played LightRush against PassiveAI leaves the recorded game
    before its last entry."""
    group = [e for e in _lr(GROUPS[(8, 8)]) if e["map"].endswith("/8x8/basesWorkers8x8.xml")]
    assert len(group) == 1
    bad = _run(group, "LightRush", "PassiveAI", stop_at_mismatch=True)
    assert bad is not None, "LightRush vs PassiveAI reproduced the LightRush vs LightRush trace"
