"""The cases of tests/test_gpu_fused_state.py: multi-step launches under unit-type tables v2 / v3, and a handle's
state changed by the host between fused launches.  GPU-free; tests/test_fused_state_cases_cpu.py keeps the cases
honest on the oracle alone (what each reaches is in DESIGN.md §4, "Fused launches under UTT v2 / v3 and across
restores").

Under v3 damage is drawn from the env's java.util.Random (UnitAction.java:24, 356-361; the state block's
H_RNG_DAMAGE words), so a case is worth something only if its launches draw: the oracle counts every stream's
draws (OracleVecClient.rng_draws).  The headline maps never draw (Workers and Bases hit for 1 in every table) and
the unmasked uniform policy never lands an attack, so neither is used here.

Game seed 5, policy seed tests.defs.SEED, slot base 0; every slot plays the masked random policy of player 0's
masks (rollout_fused's own rows, oref_rollout_policy on the oracle)."""
import numpy as np

from tests import combat_maps as C
from tests import dumps, oracle_py
from tests.defs import SEED

GAME_SEED = 5
STEPS = 220                 # the horizon of the adequacy conditions and of the multi-step comparisons
MARKS = (20, 60, 120, 220)  # where DESIGN.md records the draws
INJECT_AT, INJECT_TAIL = 60, (64, 26)  # the host changes the state at step 60; then rollouts to 124 and 150
DONOR = 2  # an injected game g takes the state of game g + DONOR (mixed_maps alternates per game: g + 1 is another map)
HEADLINE16 = "maps/16x16/basesWorkers16x16.xml"


def _case(id, maps, slots, utt, po=False, max_units=0, max_steps=2000):
    return dict(id=id, maps=maps, slots=slots, utt=utt, po=po, max_units=max_units, max_steps=max_steps)


def _fixed(mp):
    return lambda tmp_path, n: [mp] * n


def _arena(W, H):
    return lambda tmp_path, n: C.arena_maps(tmp_path, W, H, n)


# id, maps(tmp_path, slots) -> one path per slot, slots, table version, view; the instance each reaches:
#   mix16-*    the 16x16 multi-step kernel, and its steady instance on a handle without a Responses ring
#   arena8-*, melee8-v3    the 8x8 multi-step kernel
#   arena32po-v3           the 32x32 partially observable helper-wave multi-step kernel
CASES = [
    _case("mix16-v3", C.mixed_maps, 64, 3),
    _case("mix16-v2", C.mixed_maps, 64, 2),
    _case("mix16-v3-resets", C.mixed_maps, 64, 3, max_steps=40),
    _case("arena8-v3", _arena(8, 8), 64, 3),
    _case("arena8-v2", _arena(8, 8), 64, 2),
    _case("melee8-v3", _fixed(C.MELEE8), 64, 3),
    _case("arena32po-v3", _arena(32, 32), 32, 3, po=True, max_units=256),
]
BY_ID = {c["id"]: c for c in CASES}
# at least this many dones and positive WinLoss rewards within STEPS (slots counted, as a Responses ring shows them)
ENDINGS = {"mix16-v3": (2, 1), "mix16-v2": (2, 1), "arena8-v3": (2, 1), "arena8-v2": (2, 1), "arena32po-v3": (2, 1)}
MULTI_STEP = ["mix16-v3", "mix16-v2", "mix16-v3-resets", "arena8-v3", "melee8-v3", "arena32po-v3"]
AGAINST_ORACLE = ["mix16-v3", "mix16-v2", "mix16-v3-resets", "arena8-v3", "arena32po-v3"]
HOST_CHANGES = ["mix16-v3", "melee8-v3", "arena32po-v3"]
# the injected games' damage draws after the injection, at least (tests/test_fused_state_cases_cpu.py)
INJECTED_DRAWS = {"mix16-v3": 10, "melee8-v3": 20, "arena32po-v3": 5}


def oracle(case, maps, utt=None, rfs=None):
    """The oracle of a case on `maps` (utt: another table version than the case's)."""
    return oracle_py.OracleVecClient(case["slots"], 0, case["max_steps"], maps, partial_obs=case["po"],
                                     utt_version=utt or case["utt"], seed=GAME_SEED,
                                     rewards=[oracle_py.REWARD_IDS[r] for r in rfs] if rfs else None)


def handle(case, maps, **kw):
    """A device env of a case on `maps` (imports the package: GPU tests only)."""
    from microrts_amd import DeviceVecEnv, UnitTypeTable

    return DeviceVecEnv(case["slots"], 0, case["max_steps"], maps, utt=UnitTypeTable(case["utt"], 1), seed=GAME_SEED,
                        partial_obs=case["po"], max_units=case["max_units"], **kw)


def damage_draws(ref):
    """Draws so far on each game's damage stream, int64 [games]."""
    return np.array([ref.rng_draws(s)[2] for s in range(0, ref.S, 2)], np.int64)


def next_rows(ref, t):
    """The rows the masked policy draws for step t from the oracle's masks: what a fused launch leaves in env.actions."""
    m = ref.get_masks(0)
    return np.stack([oracle_py.policy(m[s], SEED, s, t, 0) for s in range(ref.S)])


def reach(case, maps, steps=STEPS, utt=None, uniform=False):
    """The case's rollout on the oracle alone, one rollout_policy(1, SEED, 0, t) per step.  -> dict: draws [games] at
    each of MARKS, dones / wins (slots, over every step), resets [games], the final state dumps."""
    ref = oracle(case, maps, utt=utt)
    ref.reset()
    G = ref.S // 2
    out = {"draws": {}, "dones": 0, "wins": 0, "resets": np.zeros(G, np.int64)}
    for t in range(steps):
        ref.rollout_policy(1, SEED, 0, t, uniform=uniform)
        out["dones"] += int(ref.done.sum())
        out["wins"] += int((ref.reward > 0).sum())
        out["resets"] += ref.done[0::2] != 0
        if t + 1 in MARKS or t + 1 == steps:
            out["draws"][t + 1] = damage_draws(ref)
    out["dumps"] = [ref.dump(s) for s in range(0, ref.S, 2)]
    ref.close()
    return out


def injected_games(n_slots):
    """Every fourth game; each has its donor g + DONOR in the handle."""
    return [g for g in range(0, n_slots // 2, 4) if g + DONOR < n_slots // 2]


def donor_states(ref):
    """{injected game: the oracle's state_json of its donor}, all read before anything is injected."""
    return {g: ref.state_json(2 * (g + DONOR)) for g in injected_games(ref.S)}


def inject(target, states):
    """The donors' states into the injected games of a device env or an oracle."""
    for g, text in states.items():
        target.set_state_json(2 * g, text)


def injection(case, maps):
    """The injection of the GPU test on the oracle alone: to INJECT_AT, every injected game takes its donor's state,
    then the steps of INJECT_TAIL.  -> dict per injected game: differs_before, equal_after (dumps.xy_free),
    left_donor (by the end), draws after the injection."""
    ref = oracle(case, maps)
    ref.reset()
    ref.rollout_policy(INJECT_AT, SEED, 0, 0)
    games = injected_games(ref.S)
    free = lambda g: dumps.xy_free(ref.dump(2 * g))  # noqa: E731
    out = {"games": games, "differs_before": [not np.array_equal(free(g), free(g + DONOR)) for g in games]}
    before = damage_draws(ref)
    inject(ref, donor_states(ref))
    out["equal_after"] = [np.array_equal(free(g), free(g + DONOR)) for g in games]
    ref.rollout_policy(sum(INJECT_TAIL), SEED, 0, INJECT_AT)
    out["left_donor"] = [not np.array_equal(free(g), free(g + DONOR)) for g in games]
    out["draws"] = (damage_draws(ref) - before)[games]
    ref.close()
    return out
