"""Combat units, ranged attacks and decisive endings on the GPU, bit-exact against the CPU oracle.

The random-policy rollouts from basesWorkers* starts never show the output kernels a Light, Heavy or
Ranged unit, an attack slot outside the centre 3x3 of the 7x7 window, a sight disk of radius 2, damage
other than 1 or a game that ends by elimination ("What the random rollouts never reach").
The scenarios of tests.combat_maps do, within 300 steps; tests/test_combat_scenarios.py keeps them
honest on the oracle alone.  Here they run through every shipped form: one launch per step against the
oracle (tests.gpu_checks.rollout: observations, masks, the 8 reward functions and dones every
step, state dumps every 10th), multi-step launches against one launch per step and against the
oracle, the records exchange and render, the one-hot encoder and the forward model."""
import numpy as np
import pytest

from tests import combat_maps as C
from tests import dumps, gpu_checks, oracle_py
from tests.defs import HEAVY, HP, LIGHT, SEED
from tests.gpu_checks import rollout
from tests.gpu_support import assert_matches_oracle, assert_same_outputs, torch_gpu

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sc", C.ROLLOUTS, ids=[s["id"] for s in C.ROLLOUTS])
def test_combat_rollout_matches_oracle(sc, tmp_path):
    """One launch per step, the masked policy, all 8 reward functions, 16 slots (8 agent-vs-RandomBiasedAI
    games for the bot handles) x 300 steps."""
    n = sc["n_slots"]
    rollout.nonzero = np.zeros(len(C.ALL_RFS), bool)
    flags = rollout(sc["maps"](tmp_path, n), n - sc["n_bot"], n_bot=sc["n_bot"], steps=sc["steps"], utt=sc["utt"],
                     crs=sc["crs"], partial_obs=sc["po"], rfs=C.ALL_RFS, max_units=sc["max_units"], players=sc["players"],
                     bots=["RandomBiasedAI"] * sc["n_bot"] if sc["n_bot"] else None, seed=C.GAME_SEED)
    assert not flags.any()
    assert rollout.nonzero[C.ALL_RFS.index("AttackRewardFunction")] or sc["kind"] == "barracks"
    if sc["kind"] == "arena":
        assert rollout.nonzero[0], "no WinLoss reward: no game ended by elimination"


# ------------------------------------------------------------------ multi-step launches
def _multi_maps(which, tmp_path, n_sp):
    if which == "mix16":
        return C.mixed_maps(tmp_path, n_sp), False, 0
    if which == "arena8":
        return C.arena_maps(tmp_path, 8, 8, n_sp), False, 0
    return C.arena_maps(tmp_path, 32, 32, n_sp), True, 256


@pytest.mark.parametrize("which,n_sp", [("mix16", 64), ("arena8", 64), ("arena32-po", 32)])
def test_multi_step_matches_single_launches(which, n_sp, tmp_path):
    """The check of tests/test_gpu_parity.py test_multi_step_rollout_matches_single_launches on handles whose
    every auto-reset inside a launch follows an elimination (max_steps 2000): arena-16x16 games mixed with
    melee16x16Mixed12 games (the 16x16 kernel and, B carrying no ring, its steady instance), arena-8x8,
    arena-32x32 partially observable (the helper-wave instance).  The one-launch-per-step twin A carries
    the Responses ring (mrts_set_step_responses), which must show at least one done."""
    torch_gpu()
    from microrts_amd import DeviceVecEnv

    maps, po, mu = _multi_maps(which, tmp_path, n_sp)
    mk = lambda: DeviceVecEnv(n_sp, 0, 2000, maps, seed=5, partial_obs=po, max_units=mu)  # noqa: E731
    A, B = mk(), mk()
    A.set_multi_step(False)
    A.set_step_responses(250)
    assert B.multi_step_capable
    for e in (A, B):
        e.reset()
        e.random_policy(SEED, 0)
    dones = wins = 0

    def same(tag):
        assert_same_outputs(A, B, tag)

    k = 0
    for n in (1, 2, 5, 64, 250):
        A.rollout_fused(SEED, k + 1, n)
        B.rollout_fused(SEED, k + 1, n)
        k += n
        same(f"after rollout to {k}")
        dones += int(A.step_dones[:n].sum())
        wins += int((A.step_rewards[:n] > 0).sum())
    for e in (A, B):
        e.step_fused(SEED, k + 1)
        e.step_fused(SEED, k + 2)
    same("after single fused steps")
    for e in (A, B):
        e.rollout_fused(SEED, k + 3, 30)
        e.step()
        e.rollout_fused(SEED, k + 40, 20)
    same("after a plain step between rollouts")
    assert dones >= 2 and wins >= 1, f"no elimination inside the launches (dones {dones}, wins {wins})"
    assert (A._h.env_steps() < 2000).all()
    assert not A.error_flags().any() and not B.error_flags().any()
    A.close()
    B.close()


def test_multi_step_mix_matches_oracle(tmp_path):
    """Multi-step launches against the oracle, as tests/test_headline_parity.py _masked_multi_step: a K = 20
    and then a K = 200 step launch on the arena / melee 16x16 mix; the oracle plays every slot with its own
    masks and its own Philox rows.  Handle E (WinLoss alone, no ring: the steady instance) is compared at
    both launch ends: observations, rewards, dones, masks, next action rows, every game's state.  Handle F
    (all 8 reward functions, a Responses ring) is compared at every step: reward / done [slots][8]."""
    torch_gpu()
    from microrts_amd import DeviceVecEnv

    S = 64
    maps = C.mixed_maps(tmp_path, S)
    E = DeviceVecEnv(S, 0, 2000, maps, seed=5)
    F = DeviceVecEnv(S, 0, 2000, maps, seed=5, rfs=C.ALL_RFS)
    assert E.fused_multi_step and F.fused_multi_step
    F.set_step_responses(200)
    ref = oracle_py.OracleVecClient(S, 0, 2000, maps, seed=5, rewards=[oracle_py.REWARD_IDS[r] for r in C.ALL_RFS])
    ref.reset()
    for e in (E, F):
        e.reset()
        e.random_policy(SEED, 0)
    t = 0
    ended = []
    for K in (20, 200):
        E.rollout_fused(SEED, t + 1, K)
        F.rollout_fused(SEED, t + 1, K)
        E.synchronize()
        F.synchronize()
        ring_r, ring_d = F.step_rewards[:K].cpu().numpy(), F.step_dones[:K].cpu().numpy()
        for j in range(K):
            m = ref.get_masks(0)
            _, rew, done = ref.step(np.stack([oracle_py.policy(m[s], SEED, s, t, 0) for s in range(S)]))
            t += 1
            assert np.array_equal(ring_r[j], rew), f"step {t}: reward\n gpu {ring_r[j]}\n ref {rew}"
            assert np.array_equal(ring_d[j], done), f"step {t}: done"
            ended += [(float(rew[s, 0]), float(rew[s + 1, 0])) for s in range(0, S, 2) if done[s, 0]]
        tag = f"after the {K}-step launch (step {t})"
        m = ref.get_masks(0)
        nxt = np.stack([oracle_py.policy(m[s], SEED, s, t, 0) for s in range(S)])
        assert_matches_oracle(E, ref, f"E {tag}", next_rows=nxt, rewards="first", states="even")
        assert_matches_oracle(F, ref, f"F {tag}", next_rows=nxt, rewards=None, states="even")
    assert (1.0, -1.0) in ended and (-1.0, 1.0) in ended, f"the launches held no decisive ending of both signs: {ended}"
    for e in (E, F):
        assert not e.error_flags().any()
        e.close()
    ref.close()


# ------------------------------------------------------------------ records, one-hot, forward model
@pytest.mark.parametrize("which", ["melee16", "skirmish32-po"])
def test_record_exchange_with_combat_units(which, tmp_path):
    """tests.gpu_checks.record_exchange_loopback_ranks (the loopback transport: every step's
    records, rendered back for every rank, equal the step's own observation) on melee16x16Mixed12 and on a
    32x32 partially observable skirmish holding Light, Heavy and Ranged units of both players: the
    receiver paints radius-2 and radius-3 sight disks from the unit-type table."""
    if which == "melee16":
        gpu_checks.record_exchange_loopback_ranks(C.MELEE16, False, 7, 8, 3)
    else:
        gpu_checks.record_exchange_loopback_ranks(C.skirmish32(tmp_path / "skirmish32.xml"), True, 9, 4, 1)


def test_onehot_encoder_with_combat_units():
    """tests.gpu_checks.onehot_encoder on melee16x16Mixed12: type-plane values 5 .. 7 and
    hp values above 1 in the one-hot layout."""
    gpu_checks.onehot_encoder(C.MELEE16, False)


def test_playouts_with_damaged_units_match_oracle():
    """tests/test_forward_model.py test_gpu_playouts_match_oracle on melee8x8Mixed6: playouts and
    mrts_evaluate (SimpleSqrtEvaluationFunction3.java:24-44) with Heavy and Light units at 0 < hp < maxhp,
    so the sqrt(hp / maxhp) terms are evaluated away from 1; state dumps and float32 values bit-exact."""
    torch_gpu()
    from microrts_amd import ForwardModel

    n = 16
    ai1, ai2, n1, n2 = gpu_checks.fm_mixed(n)
    gpu = ForwardModel(n, C.MELEE8, policies=(n1, n2), seed=21)
    ref = oracle_py.OracleForwardModel(n, C.MELEE8, ai1, ai2, seed=21)
    gpu_checks.fm_compare(gpu, ref, n, "initial")
    damaged = 0
    for chunk, horizon in enumerate([0, 1, 13, 30, 30, 30, 50, 100]):
        gpu.playout(horizon)
        for g in range(n):
            ref.playout(g, horizon)
            u = dumps.live_units(ref.dump(g))
            damaged += int(((np.isin(u[:, 0], (LIGHT, HEAVY))) & (u[:, 4] > 0) & (u[:, 4] < HP[LIGHT])).sum())
        gpu_checks.fm_compare(gpu, ref, n, f"chunk {chunk} (horizon {horizon})")
    assert damaged >= 10, f"the evaluated states held too few damaged Light / Heavy units ({damaged})"
    gpu.close()
    ref.close()
