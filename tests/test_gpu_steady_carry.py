"""What the steady instance of the 16x16 multi-step step kernel carries from one step of a launch to the next
(DESIGN.md §5p): the issue index (`bits`, the PRODUCE cost sums and maxima), the sampled action in decoded form,
and the game's outcome.  The general instance re-derives all three every step, so it is the reference.

The method is tests/test_gpu_steady_instance.py's: two handles with the same seed make the same rollout_fused
calls, set_step_responses(ring) holds one of them on the general instance, and after every call everything a
launch leaves is compared bit for bit (observations, masks, next action rows, source bits, rewards, dones, error
flags, env steps, every game's state dump).  16x16 is the only shape the instance runs.  The cases
(tests/steady_carry_cases.py) are chosen for what removes assignments between two steps of a launch: kills of
units with pending MOVEs / PRODUCEs, overlapping productions, auto-resets inside a launch, and the merged issue
pass's fall-backs; tests/test_steady_carry_cases_cpu.py asserts on the oracle alone that they reach them.  Two
cases are also stepped against the CPU oracle for their first 30 steps.

With the audit build (MRTS_LIB_PATH=microrts_amd/libmrts_audit.so) every carried step also rebuilds the index
the old way and compares; a mismatch sets error flag bit 7, which the error-flag assertion here reports.
"""
import numpy as np
import pytest

from tests import oracle_py
from tests import steady_carry_cases as C
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
            e.set_state_json(2 * g, C.injected_state())
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
            ref.set_state_json(2 * g, C.injected_state())
    for step in range(n):
        m = ref.get_masks(0)
        ref.step(np.stack([oracle_py.policy(m[s], SEED, s, step, 0) for s in range(S)]))
    m = ref.get_masks(0)
    nxt = np.stack([oracle_py.policy(m[s], SEED, s, n, 0) for s in range(8)])
    assert_matches_oracle(E, ref, tag, next_rows=nxt, states="even", xy_free=True, env_steps=True)
    ref.close()


@pytest.mark.parametrize("name", list(C.CASES))
def test_carried_state_equals_rederived(name):
    torch_gpu()
    c = C.CASES[name]
    A, B = _env(c, False), _env(c, True)
    assert_same_outputs(A, B, f"{name}: before the first call")
    n_or = c["oracle_steps"]
    k = 0
    for n in c["calls"]:
        A.rollout_fused(SEED, k + 1, n)
        B.rollout_fused(SEED, k + 1, n)
        k += n
        assert_same_outputs(A, B, f"{name}: after the call to step {k}")
        if k == n_or:  # the steady handle itself, where its first call ends at the oracle's horizon
            _against_oracle(A, c, n_or, f"{name}: steady vs oracle after {n_or} steps")
    if n_or and n_or not in np.cumsum(c["calls"]):
        # the case's calls do not end there (one call of 90 keeps the resets strictly inside the launch): a third
        # handle, same seed, runs the steady instance for the oracle's horizon alone
        O = _env(c, False)
        O.rollout_fused(SEED, 1, n_or)
        _against_oracle(O, c, n_or, f"{name}: steady vs oracle after {n_or} steps")
        O.close()
    if c["max_steps"] < k:
        assert (A._h.env_steps() == k % c["max_steps"]).all(), "no auto-reset happened"
    A.close()
    B.close()
