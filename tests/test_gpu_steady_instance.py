"""The steady instance of the 16x16 multi-step step kernel (k_env STEADY) against the general one.

launchEnv runs the steady instance when a fused self-play rollout on the 16x16 shape is in its steady state
(steadyLaunch in mrts_kernels.hip): the option tests such a launch never changes are compile-time constants
there.  Both instances must compute the same thing.  A handle is kept off the steady instance by an option
that changes no result: set_step_responses(K) makes every launch write its rewards / dones into a ring
(KDyn.resp_stride != 0), whose last entry env.reward / env.done then show.  Everything a launch leaves is
compared after every call: observations, masks, next action rows, rewards, dones, error flags and every
game's state dump.
"""
import ctypes

import pytest

from tests.defs import SEED
from tests.gpu_support import assert_same_outputs, torch_gpu

MAP = "maps/16x16/basesWorkers16x16.xml"

# mrts_internal_steady_probe's deviations from the steady state, in its order (mrts_kernels.hip)
DEVIATIONS = ["n_iter == 1", "8x8 shape", "partial observability", "a bot game", "a LightRush handle", "mask_delta off",
              "pol_delta off", "fwd_read off", "obs_img off", "no obs", "no masks", "no source", "no pol_actions", "no reward",
              "no done", "no prio_tab", "no bal", "obs8", "obs16", "rec_out", "uni_actions", "rows", "resp_stride", "two rewards",
              "another reward kind", "reward bookkeeping", "no actions"]


def test_predicate_picks_the_general_instance_for_every_single_deviation():
    """steadyLaunch (launchEnv's selection) on the CPU: the steady state itself is accepted, and each condition
    the instance compiles as a constant, changed alone, sends the launch to the general instance."""
    from microrts_amd import _lib

    probe = _lib.load().mrts_internal_steady_probe  # (the loader: torch's HIP runtime first, one per process)
    probe.argtypes, probe.restype = [ctypes.c_int], ctypes.c_int
    assert probe(-1) == 1, "the steady state itself"
    for k, what in enumerate(DEVIATIONS):
        assert probe(k) == 0, f"deviation {k} ({what}) still selects the steady instance"
    assert probe(len(DEVIATIONS)) == -1, "the library knows a deviation this test does not name"


def _env(S, max_steps, general, ring):
    from microrts_amd import DeviceVecEnv

    e = DeviceVecEnv(S, 0, max_steps, [MAP] * S, seed=3)
    assert e.fused_multi_step
    if general:
        e.set_step_responses(ring)
    e.reset()
    e.random_policy(SEED, 0)
    return e


# (slots, max_steps, steps of each call): 3 games x 2 calls of 5 — not a multiple of 512 games, no balanced
# placement; 512 games x 70 steps — balanced placement on, and 70 >= BAL_MIN_ITER = 64, so the first steady launch
# of 64 steps writes a permutation that the later launches use; 512 games with max_steps = 40 over 90 steps —
# every game auto-resets inside the launches
SHAPES = {"6x5": (12, 2000, (5, 5)), "512x70": (1024, 2000, (70, 70)), "512x90_resets": (1024, 40, (90,))}


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_steady_equals_general(shape):
    """Two handles, same seed, same rollout_fused calls: one in the steady state, one held on the general instance."""
    torch_gpu()
    S, max_steps, calls = SHAPES[shape]
    A, B = _env(S, max_steps, False, max(calls)), _env(S, max_steps, True, max(calls))
    assert_same_outputs(A, B, f"{shape}: after reset")
    k = 0
    for n in calls:
        A.rollout_fused(SEED, k + 1, n)
        B.rollout_fused(SEED, k + 1, n)
        k += n
        assert_same_outputs(A, B, f"{shape}: after the call to step {k}")
    if max_steps < k:
        assert (A._h.env_steps() < max_steps).all() and (A._h.env_steps() == k % max_steps).all(), "no auto-reset happened"
    A.close()
    B.close()


@pytest.mark.gpu
def test_one_handle_alternating_instances():
    """steady -> general -> steady on one handle, mid-episode, against a twin that stays general: the forwarded
    action rows, the mask row sets and the game placement carry over between the instances."""
    torch_gpu()
    S, ring = 1024, 70
    A, B = _env(S, 2000, False, ring), _env(S, 2000, True, ring)
    k = 0
    for n, general in ((70, False), (33, True), (70, False), (7, True), (20, False)):
        A.set_step_responses(ring if general else 0)
        A.rollout_fused(SEED, k + 1, n)
        B.rollout_fused(SEED, k + 1, n)
        k += n
        assert_same_outputs(A, B, f"after the {'general' if general else 'steady'} call to step {k}")
    A.close()
    B.close()
