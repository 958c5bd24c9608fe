"""The mask pass of the steady instance of the 16x16 multi-step step kernel: own idle units and the
cells idle units have left go through one list of quads — four lanes compute a unit's mask row, store its record from
their registers, sample its next action row and post the decoded row to the unit's lane; a vacated cell is an entry
with a zero row.  The general instance lists and stores them in separate passes, so it is the reference.

The method is tests/test_gpu_steady_cycle.py's: two handles with the same seed make the same rollout_fused calls,
set_step_responses(ring) holds one of them on the general instance, and after every call everything a launch leaves
is compared bit for bit (observations, masks, next action rows, source bits, rewards, dones, error flags, env steps,
every game's state dump).  The cases (tests/steady_masks_cases.py) put more than 16 idle units and more than 16 / 32
list entries into one game, idle Ranged units at the left and top edges, a player's resources across a unit cost in
both directions under an idle Base, game overs and max_steps resets on a call's last step and one before it behind
many idle units, and a game that passes 64 units and comes back; tests/test_steady_masks_cases_cpu.py asserts on the
oracle alone that they do, on steps the steady instance runs (a handle's first launch after an injection is a single
step of the general kernel).  Three cases are also stepped against the CPU oracle for their first 30 steps."""
import numpy as np
import pytest

from tests import oracle_py
from tests import steady_masks_cases as C
from tests.gpu_support import assert_matches_oracle, assert_same_outputs, torch_gpu

pytestmark = pytest.mark.gpu

SEED = C.SEED


def _env(name, general):
    from microrts_amd import DeviceVecEnv

    c = C.CASES[name]
    S = 2 * C.GAMES
    e = DeviceVecEnv(S, 0, c["max_steps"], [C.MAP16] * S, seed=C.GAME_SEED)
    assert e.fused_multi_step
    if general:
        e.set_step_responses(max(c["calls"]))
    e.reset()
    for g in range(C.GAMES):
        e.set_state_json(2 * g, C.injected(name, g))
    e.get_masks()
    e.random_policy(SEED, 0)
    return e


def _against_oracle(E, name, n, tag):
    """Handle E after its first n steps against the oracle's n steps from the same start."""
    c = C.CASES[name]
    S = 2 * C.GAMES
    ref = oracle_py.OracleVecClient(S, 0, c["max_steps"], [C.MAP16] * S, seed=C.GAME_SEED)
    ref.reset()
    for g in range(C.GAMES):
        ref.set_state_json(2 * g, C.injected(name, g))
    for step in range(n):
        m = ref.get_masks(0)
        ref.step(np.stack([oracle_py.policy(m[s], SEED, s, step, 0) for s in range(S)]))
    m = ref.get_masks(0)
    nxt = np.stack([oracle_py.policy(m[s], SEED, s, n, 0) for s in range(S)])
    assert_matches_oracle(E, ref, tag, next_rows=nxt, states="even", xy_free=True, env_steps=True)
    ref.close()


@pytest.mark.parametrize("name", list(C.CASES))
def test_steady_masks_equal_general(name):
    torch_gpu()
    c = C.CASES[name]
    assert 2 in c["calls"] and 3 in c["calls"] and sum(c["calls"]) <= 60
    A, B = _env(name, False), _env(name, True)
    assert_same_outputs(A, B, f"{name}: before the first call")
    k = 0
    for n in c["calls"]:
        A.rollout_fused(SEED, k + 1, n)
        B.rollout_fused(SEED, k + 1, n)
        k += n
        assert_same_outputs(A, B, f"{name}: after the call to step {k}")
    n_or = c["oracle_steps"]
    if n_or:  # a third handle, same seed, runs the steady instance for the oracle's horizon alone
        O = _env(name, False)
        O.rollout_fused(SEED, 1, n_or)
        _against_oracle(O, name, n_or, f"{name}: steady vs oracle after {n_or} steps")
        O.close()
    A.close()
    B.close()
