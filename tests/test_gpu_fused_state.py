"""The fused multi-step launches under unit-type tables v2 / v3, and a handle's state changed by the host between
fused launches.  The cases are tests.fused_state_cases; tests/test_fused_state_cases_cpu.py shows on the oracle alone
that each draws random damage inside the compared launches.

First half.  Every other multi-step test builds its handles with table v1, and v2 / v3 were stepped one launch per
step only.  Under v3 every game's damage stream (the state block's H_RNG_DAMAGE words; UnitAction.java:24, 356-361)
must pass from step to step inside a launch, go on across the in-launch auto-reset (the oracle seeds it once per env)
and be written back at the launch's end; under v2 the steady instance's carried PRODUCE cost sums follow other costs.
The bodies are those of tests/test_gpu_combat.py: multi-step against one launch per step, and against the oracle.

Second half.  After fused launches a handle holds caches beside the state blocks: the masks' and source bits' delta
base, the policy's, the forwarded action words and their launch stamp, the partially observable render records and,
from 512 games up, a balanced-placement permutation.  mrts_restore, mrts_set_state_json and mrts_reset_dev change the
state behind them; every other test of those does so before the first fused launch or on handles that run one launch
per step.  Here they happen at step 60 of a fused pipeline, followed by the documented protocol (get_masks(),
random_policy(SEED, k), rollout_fused(SEED, k + 1, n)), and the outcome is compared with the same handle's own
uninterrupted run, with a twin held to one launch per step and with the oracle.  One test leaves the protocol out:
get_masks() and random_policy() drop the forwarded action words themselves, so only a rollout_fused right after the
injection shows that mrts_set_state_json dropped them."""
import pytest

from tests import fused_state_cases as F
from tests.defs import SEED
from tests.combat_maps import ALL_RFS
from tests.gpu_support import Record, assert_matches_oracle, assert_same_outputs, same, torch_gpu

pytestmark = pytest.mark.gpu


def _maps(cid, tmp_path):
    c = F.BY_ID[cid]
    return c, c["maps"](tmp_path, c["slots"])


def _start(e):
    e.reset()
    e.random_policy(SEED, 0)


def _roll(envs, k, n):
    """rollout_fused of n steps from step index k on each env -> k + n"""
    for e in envs:
        e.rollout_fused(SEED, k + 1, n)
    return k + n


def _resume(envs, k):
    """The documented protocol after the host changed the state: the masks, then the rows of step index k."""
    for e in envs:
        e.get_masks()
        e.random_policy(SEED, k)


def _close(*things):
    for t in things:
        t.close()


# ------------------------------------------------------------------ first half: tables v2 / v3
@pytest.mark.parametrize("cid", F.MULTI_STEP)
def test_multi_step_matches_single_launches(cid, tmp_path):
    """tests/test_gpu_combat.py test_multi_step_matches_single_launches under v2 / v3: twin A one launch per step with a
    Responses ring, twin B multi-step (on mix16-* the steady instance: B carries no ring).  A under v3 is itself
    compared with the oracle by the arena16-utt3 / melee8-utt3-* rollouts of tests.combat_maps.ROLLOUTS."""
    torch_gpu()
    c, maps = _maps(cid, tmp_path)
    A, B = F.handle(c, maps), F.handle(c, maps)
    A.set_multi_step(False)
    A.set_step_responses(150)
    assert B.fused_multi_step
    _start(A)
    _start(B)
    dones = wins = k = 0
    for n in (1, 2, 5, 64, 148):
        k = _roll((A, B), k, n)
        assert_same_outputs(A, B, f"{cid}: after the rollout to {k}")
        dones += int(A.step_dones[:n].sum())
        wins += int((A.step_rewards[:n] > 0).sum())
    assert k == F.STEPS
    for e in (A, B):
        e.step_fused(SEED, k + 1)
        e.step_fused(SEED, k + 2)
    assert_same_outputs(A, B, f"{cid}: after single fused steps")
    for e in (A, B):
        e.rollout_fused(SEED, k + 3, 30)
        e.step()
        e.rollout_fused(SEED, k + 40, 20)
    assert_same_outputs(A, B, f"{cid}: after a plain step between rollouts")
    if cid in F.ENDINGS:
        assert dones >= F.ENDINGS[cid][0] and wins >= F.ENDINGS[cid][1], f"{cid}: dones {dones}, wins {wins} inside the launches"
    if c["max_steps"] < F.STEPS:
        assert dones >= 5 * c["slots"], f"{cid}: {dones} dones: not every game reset 5 times inside the launches"
    assert (A._h.env_steps() < c["max_steps"]).all()
    _close(A, B)


@pytest.mark.parametrize("cid", F.AGAINST_ORACLE)
def test_multi_step_matches_oracle(cid, tmp_path):
    """tests/test_gpu_combat.py test_multi_step_mix_matches_oracle under v2 / v3: a K = 20 and then a K = 200 launch.
    Handle E (WinLoss alone, no ring: on mix16-* the steady instance) and handle F (all 8 reward functions, a ring)
    against the oracle at both launch ends (observations, masks, next action rows, every game's state, env steps),
    F's ring against the oracle's reward / done of every step."""
    torch_gpu()
    c, maps = _maps(cid, tmp_path)
    E, Fh = F.handle(c, maps), F.handle(c, maps, rfs=ALL_RFS)
    assert E.fused_multi_step and Fh.fused_multi_step
    Fh.set_step_responses(200)
    ref = F.oracle(c, maps, rfs=ALL_RFS)
    ref.reset()
    _start(E)
    _start(Fh)
    t = 0
    for K in (20, 200):
        _roll((E, Fh), t, K)
        Fh.synchronize()
        ring_r, ring_d = Fh.step_rewards[:K].cpu().numpy(), Fh.step_dones[:K].cpu().numpy()
        for j in range(K):
            ref.rollout_policy(1, SEED, 0, t)
            t += 1
            assert (ring_r[j] == ref.reward).all(), f"{cid} step {t}: reward\n gpu {ring_r[j]}\n ref {ref.reward}"
            assert (ring_d[j] == ref.done).all(), f"{cid} step {t}: done"
        tag = f"{cid}: after the {K}-step launch (step {t})"
        nxt = F.next_rows(ref, t)
        assert_matches_oracle(E, ref, f"E {tag}", next_rows=nxt, rewards="first", states="even", env_steps=True)
        assert_matches_oracle(Fh, ref, f"F {tag}", next_rows=nxt, rewards=None, states="even", env_steps=True)
    for e in (E, Fh):
        assert not e.error_flags().any()
    _close(E, Fh, ref)


# ------------------------------------------------------------------ second half: the host changes the state
def _to_checkpoint(c, maps, twin=False):
    """A handle (and its one-launch-per-step twin) run to step 60 by fused rollouts of 20 and 40 steps, their
    checkpoints there, and the records X of the uninterrupted run at steps 124 and 150.
    -> (envs, checkpoints, (X124, X150))"""
    envs = [F.handle(c, maps)] + ([F.handle(c, maps)] if twin else [])
    assert envs[0].fused_multi_step
    if twin:
        envs[1].set_multi_step(False)
    for e in envs:
        _start(e)
    k = _roll(envs, 0, 20)
    k = _roll(envs, k, 40)
    assert k == F.INJECT_AT
    cks = [e.checkpoint() for e in envs]
    X = []
    for n in F.INJECT_TAIL:
        k = _roll(envs, k, n)
        X.append(Record(envs[0]))
        for e in envs[1:]:
            assert_same_outputs(e, X[-1], f"{c['id']}: the twin at step {k}")
    return envs, cks, X


def _replay(e, X, tag):
    """From a restored step-60 state: the protocol and the same two rollouts; both points must equal X."""
    _resume([e], F.INJECT_AT)
    k = F.INJECT_AT
    for n, x in zip(F.INJECT_TAIL, X):
        k = _roll([e], k, n)
        assert_same_outputs(e, x, f"{tag}: step {k} against the uninterrupted run")


@pytest.mark.parametrize("cid", F.HOST_CHANGES)
def test_checkpoint_and_replay(cid, tmp_path):
    """restore() at step 150 of a fused pipeline of the checkpoint taken at step 60: the replay gives the first run's
    outputs at steps 124 and 150, on the multi-step handle and on its one-launch-per-step twin; and an oracle stepped
    150 times from the start equals the restored handle (the v3 damage stream travels in the checkpoint)."""
    torch_gpu()
    c, maps = _maps(cid, tmp_path)
    (H, T), (ckH, ckT), X = _to_checkpoint(c, maps, twin=True)
    H.restore(ckH)
    T.restore(ckT)
    _replay(H, X, f"{cid}: restored")
    _replay(T, X, f"{cid}: restored twin")
    ref = F.oracle(c, maps)
    ref.reset()
    k = F.INJECT_AT + sum(F.INJECT_TAIL)
    ref.rollout_policy(k, SEED, 0, 0)
    assert_matches_oracle(H, ref, f"{cid}: restored, step {k}", next_rows=F.next_rows(ref, k), states="even", env_steps=True)
    _close(H, T, ref)


@pytest.mark.parametrize("cid", F.HOST_CHANGES)
def test_restore_into_another_handle(cid, tmp_path):
    """The step-60 checkpoint into a handle of the same configuration that was never reset, and into one that has
    run other launches (other launch stamps, delta bases and forwarded rows): both replay the first handle's run."""
    torch_gpu()
    c, maps = _maps(cid, tmp_path)
    (H,), (ck,), X = _to_checkpoint(c, maps)
    fresh, used = F.handle(c, maps), F.handle(c, maps)
    _start(used)
    k = _roll([used], 0, 7)
    _roll([used], k, 30)
    for name, e in (("a handle never reset", fresh), ("a handle that ran 37 steps", used)):
        e.restore(ck)
        _replay(e, X, f"{cid}: {name}")
    _close(H, fresh, used)


def test_restore_after_the_placement_permutation_exists():
    """basesWorkers16x16, 512 games (tests/test_gpu_steady_instance.py "512x70"): the first steady launch of at least
    64 steps writes the balanced-placement permutation, which a restore leaves in place while the games under it
    change.  Restore and replay give the first run's outputs; so does a fresh handle, which has no permutation until
    its own first long launch."""
    torch_gpu()
    from microrts_amd import DeviceVecEnv

    S, n = 1024, 70
    mk = lambda: DeviceVecEnv(S, 0, 2000, [F.HEADLINE16] * S, seed=F.GAME_SEED)  # noqa: E731
    H = mk()
    assert H.fused_multi_step
    _start(H)
    k = _roll([H], 0, n)
    ck = H.checkpoint()
    _roll([H], k, n)
    X = Record(H)
    fresh = mk()
    for name, e in (("the same handle", H), ("a fresh handle", fresh)):
        e.restore(ck)
        _resume([e], k)
        _roll([e], k, n)
        assert_same_outputs(e, X, f"{name}: step {k + n} against the uninterrupted run")
    _close(H, fresh)


@pytest.mark.parametrize("cid", F.HOST_CHANGES)
def test_injection_mid_pipeline(cid, tmp_path):
    """At step 60 of a fused pipeline every fourth game of the handle, of its one-launch-per-step twin and of the oracle
    takes the oracle's state_json of game g + 2 (another arena variant on the mixed maps: the terrain changes too);
    the other games go on untouched.  After the protocol, rollouts of 64 and 26 steps: the handle equals the twin and
    the oracle after each, no error flag."""
    torch_gpu()
    c, maps = _maps(cid, tmp_path)
    H, T = F.handle(c, maps), F.handle(c, maps)
    assert H.fused_multi_step
    T.set_multi_step(False)
    ref = F.oracle(c, maps)
    ref.reset()
    _start(H)
    _start(T)
    k = _roll((H, T), 0, 20)
    k = _roll((H, T), k, 40)
    ref.rollout_policy(k, SEED, 0, 0)
    assert_matches_oracle(H, ref, f"{cid}: before the injection", next_rows=F.next_rows(ref, k), states="even", env_steps=True)
    states = F.donor_states(ref)
    for target in (H, T, ref):
        F.inject(target, states)
    _resume((H, T), k)
    for n in F.INJECT_TAIL:
        _roll((H, T), k, n)
        ref.rollout_policy(n, SEED, 0, k)
        k += n
        assert_same_outputs(H, T, f"{cid}: injected, step {k}")
        assert_matches_oracle(H, ref, f"{cid}: injected, step {k}", next_rows=F.next_rows(ref, k), states="even", xy_free=True,
                              env_steps=True)
    assert not H.error_flags().any() and not T.error_flags().any()
    _close(H, T, ref)


@pytest.mark.parametrize("cid", F.HOST_CHANGES)
def test_injection_without_the_protocol(cid, tmp_path):
    """The injection followed by rollout_fused at once: get_masks() and random_policy() themselves drop the forwarded
    action words and the policy's delta base, so after the protocol nothing shows whether mrts_set_state_json did.
    Without it the first step decodes env.actions as it stands (the rows drawn at step 60 for the games as they were:
    what an injected game cannot execute is refused, as for any caller's rows) and must not take the forwarded words,
    which belong to the units the game no longer has.  The oracle steps once on those rows, then on its own policy's."""
    torch_gpu()
    c, maps = _maps(cid, tmp_path)
    H, T = F.handle(c, maps), F.handle(c, maps)
    T.set_multi_step(False)
    ref = F.oracle(c, maps)
    ref.reset()
    _start(H)
    _start(T)
    k = _roll((H, T), 0, 20)
    k = _roll((H, T), k, 40)
    ref.rollout_policy(k, SEED, 0, 0)
    rows = F.next_rows(ref, k)
    same(H.actions, rows.astype("int32"), "the rows of step 60", f"{cid}: before the injection")
    states = F.donor_states(ref)
    for target in (H, T, ref):
        F.inject(target, states)
    n = F.INJECT_TAIL[0]
    _roll((H, T), k, n)
    ref.step(rows)
    ref.rollout_policy(n - 1, SEED, 0, k + 1)
    k += n
    assert_same_outputs(H, T, f"{cid}: injected, no protocol, step {k}")
    assert_matches_oracle(H, ref, f"{cid}: injected, no protocol, step {k}", next_rows=F.next_rows(ref, k), states="even",
                          xy_free=True, env_steps=True)
    assert not H.error_flags().any() and not T.error_flags().any()
    _close(H, T, ref)


def test_uniform_rollout_resets_to_the_maps_own_walls(tmp_path):
    """The 8x8 uniform rollout, whose observations a helper wave stores (the terrain plane with a launch's first step
    only): arena-8x8 games take the state of another arena variant, other walls with it, and time out (max_steps 12)
    on the second step of a later launch.  At that launch's end the terrain plane shows the map's own walls again, as
    the oracle's does (PhysicalGameState.load on every reset), and everything else matches too."""
    torch_gpu()
    c = dict(F.BY_ID["arena8-v3"], max_steps=12)
    maps = c["maps"](tmp_path, c["slots"])
    H = F.handle(c, maps, with_masks=False)
    assert H.multi_step_capable
    ref = F.oracle(c, maps)
    H.reset()
    ref.reset()
    own = ref.obs[:, 5].copy()
    k = 0
    for n, inject in ((5, True), (10, False), (9, False)):  # the injected games' 12th step is the last launch's second
        H.rollout_uniform(SEED, k, n)
        ref.rollout_policy(n, SEED, 0, k, uniform=True)
        k += n
        assert_matches_oracle(H, ref, f"uniform, step {k}", masks=None, states="even", xy_free=True, env_steps=True)
        if inject:
            states = F.donor_states(ref)
            F.inject(H, states)
            F.inject(ref, states)
    games = F.injected_games(ref.S)
    assert all(ref.env_steps(2 * g) == 7 for g in games), [ref.env_steps(2 * g) for g in games]
    assert all((ref.obs[2 * g, 5] == own[2 * g]).all() and (own[2 * g] != own[2 * g + 2 * F.DONOR]).any() for g in games), \
        "the oracle's injected games do not show their own walls, or the donors' walls are the same"
    assert not H.error_flags().any()
    _close(H, ref)


@pytest.mark.parametrize("cid", F.HOST_CHANGES)
def test_reset_mid_pipeline(cid, tmp_path):
    """reset() at step 60 of a fused pipeline, then random_policy(SEED, 0) and a 64-step rollout: the handle equals its
    one-launch-per-step twin and an oracle reset at the same point, whose random streams go on (oref_reset reseeds
    nothing: the Java streams are statics that outlive a game)."""
    torch_gpu()
    c, maps = _maps(cid, tmp_path)
    H, T = F.handle(c, maps), F.handle(c, maps)
    T.set_multi_step(False)
    ref = F.oracle(c, maps)
    ref.reset()
    _start(H)
    _start(T)
    k = _roll((H, T), 0, 20)
    k = _roll((H, T), k, 40)
    ref.rollout_policy(k, SEED, 0, 0)
    for e in (H, T):
        _start(e)
    ref.reset()
    same(H.obs, ref.obs, "obs", f"{cid}: after the reset")
    n = 64
    _roll((H, T), 0, n)
    ref.rollout_policy(n, SEED, 0, 0)
    assert_same_outputs(H, T, f"{cid}: {n} steps after the reset")
    assert_matches_oracle(H, ref, f"{cid}: {n} steps after the reset", next_rows=F.next_rows(ref, n), states="even",
                          env_steps=True)
    _close(H, T, ref)
