"""What the steady instance of the 16x16 multi-step step kernel does differently inside a step: a
cycle's ready MOVEs execute in one lane-parallel pass unless an ATTACK is ready with them, and the reward / done
values are stored on a launch's first step and on change only.  The general instance executes every ready assignment
one by one and writes reward / done every step, so it is the reference.

The method is tests/test_gpu_steady_carry.py's: two handles with the same seed make the same rollout_fused calls,
set_step_responses(ring) holds one of them on the general instance, and after every call everything a launch leaves
is compared bit for bit (observations, masks, next action rows, source bits, rewards, dones, error flags, env steps,
every game's state dump).  Before every call the steady handle's reward / done tensors are overwritten with garbage:
the launch's first step has to write them whole.  The cases (tests/steady_cycle_cases.py) reach several MOVEs in one
cycle, MOVEs beside PRODUCEs / HARVESTs / RETURNs, MOVEs beside ATTACKs in both sequence orders, a mover killed in the
cycle of its MOVE, MOVEs onto the cell a depleted resource left, and game overs and max_steps resets on, one step
before and two steps before a call's last step; tests/test_steady_cycle_cases_cpu.py asserts on the oracle alone that
they do — the injected ATTACK / MOVE pairs on the case's second step, since a handle's first launch after a reset or an
injection is a single step of the general kernel and the steady instance runs from the second step on.  Three cases
are also stepped against the CPU oracle for their first 30 steps."""
import numpy as np
import pytest

from tests import oracle_py
from tests import steady_cycle_cases as C
from tests.gpu_support import assert_matches_oracle, assert_same_outputs, torch_gpu

pytestmark = pytest.mark.gpu

SEED = C.SEED


def _env(c, general):
    from microrts_amd import DeviceVecEnv

    S = 2 * C.GAMES
    e = DeviceVecEnv(S, 0, c["max_steps"], [c["map"]] * S, seed=C.GAME_SEED)
    assert e.fused_multi_step
    if general:
        e.set_step_responses(max(c["calls"]))
    e.reset()
    if c["inject"]:
        for g in range(C.GAMES):
            e.set_state_json(2 * g, C.injected(c["inject"]))
        e.get_masks()
    e.random_policy(SEED, 0)
    return e


def _against_oracle(E, c, n, tag):
    """Handle E after its first n steps against the oracle's n steps from the same start."""
    S = 2 * C.GAMES
    ref = oracle_py.OracleVecClient(S, 0, c["max_steps"], [c["map"]] * S, seed=C.GAME_SEED)
    ref.reset()
    if c["inject"]:
        for g in range(C.GAMES):
            ref.set_state_json(2 * g, C.injected(c["inject"]))
    for step in range(n):
        m = ref.get_masks(0)
        ref.step(np.stack([oracle_py.policy(m[s], SEED, s, step, 0) for s in range(S)]))
    m = ref.get_masks(0)
    nxt = np.stack([oracle_py.policy(m[s], SEED, s, n, 0) for s in range(8)])
    assert_matches_oracle(E, ref, tag, next_rows=nxt, states="even", xy_free=True, env_steps=True)
    ref.close()


def _garbage(E):
    """The plain reward / done tensors of a handle without a Responses ring, overwritten by the caller."""
    assert E._ring_last is None
    E.synchronize()
    E.reward.fill_(-7.5)
    E.done.fill_(0xA5)
    E.synchronize()


@pytest.mark.parametrize("name", list(C.CASES))
def test_steady_cycle_equals_general(name):
    torch_gpu()
    c = C.CASES[name]
    A, B = _env(c, False), _env(c, True)
    assert_same_outputs(A, B, f"{name}: before the first call")
    k = 0
    for n in c["calls"]:
        _garbage(A)
        A.rollout_fused(SEED, k + 1, n)
        B.rollout_fused(SEED, k + 1, n)
        k += n
        assert_same_outputs(A, B, f"{name}: after the call to step {k}")
    n_or = c["oracle_steps"]
    if n_or:  # a third handle, same seed, runs the steady instance for the oracle's horizon alone
        O = _env(c, False)
        _garbage(O)
        O.rollout_fused(SEED, 1, n_or)
        _against_oracle(O, c, n_or, f"{name}: steady vs oracle after {n_or} steps")
        O.close()
    if c["max_steps"] < k:
        assert (A._h.env_steps() == k % c["max_steps"]).all(), "no auto-reset happened"
    A.close()
    B.close()
