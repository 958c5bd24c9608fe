"""The per-game error flags (MRTS_ERR_*, state-header word H_ERR) on the GPU: each of the step kernels' error
branches is reached from the states of tests/error_cases.py (tests/test_error_cases_cpu.py shows on the oracle alone
that each scenario happens, and which of cycle()'s three paths its unit counts lead to), and the flag is asserted by
value: exactly that bit, on exactly the slots of the faulty games.

Every handle holds 8 games; games 2 and 5 get the faulty state, the others are states of recorded games and act as
controls: a fault of one game must not show in its neighbours.  Every comparison is equality (tests/gpu_support.py).

* MRTS_ERR_NEG_RESOURCES  Java prints and goes on, and so does the oracle: full parity with it from the faulty state,
  through the generic kernel, bot envs, the specialised 16x16 / 8x8 / 32x32-PO instances and the multi-step launches
  (the flag is raised in the middle of one); the flag survives the in-step auto-reset and reset() clears it.
* MRTS_ERR_ADDUNIT        Java throws; the reference is the oracle on the NONE twin (nothing produced, nothing paid).
* MRTS_ERR_MOVE_COLLISION the game is outside every contract afterwards: the controls stay exact, reset() restores all.
* MRTS_ERR_CAPACITY       64 births fill the unit slots exactly and raise nothing; of 66 the last two are refused.
* MRTS_ERR_OLDER_CONFLICT through ForwardModel.trace_step, the branch's only door.
* the host-pointer calls' return codes: -EFAULT, -ENOSPC, -EINVAL first, and that a failing call fails until reset."""
import ctypes
import os

import numpy as np
import pytest

from tests import dumps, oracle_py
from tests import error_cases as EC
from tests import state_cases as SC
from tests.defs import NONE, PRODUCE, RIGHT
from tests.gpu_support import assert_matches_oracle, same, torch_gpu
from tests.trace_fixtures import check_vs_trace, issue_rows, parse

pytestmark = pytest.mark.gpu

SEED = SC.SEED
STEPS = 25
MAX_STEPS = 14  # envSteps restarts at 0 on injection: every game times out and resets inside the 25 steps
TRACE_ISSUED = 1
EFAULT, ENOSPC, EINVAL = -14, -28, -22


def _env(size, states, max_steps=2000, bots=False, po=False, max_units=0, **kw):
    """A device env of these games (two self-play slots per game, or one bot env per game), reset, states injected"""
    from microrts_amd import DeviceVecEnv

    n, mp = len(states), EC.MAPS[size]
    if bots:
        e = DeviceVecEnv(0, n, max_steps, [mp] * n, ai2s=["RandomBiasedAI"] * n, seed=SC.GAME_SEED, partial_obs=po,
                         max_units=max_units, **kw)
    else:
        e = DeviceVecEnv(2 * n, 0, max_steps, [mp] * (2 * n), seed=SC.GAME_SEED, partial_obs=po, max_units=max_units, **kw)
    e.reset()
    for g, j in enumerate(states):
        e.set_state_json((1 if bots else 2) * g, j)
    e.get_masks()
    return e


def _bad_slots(bots=False):
    return list(EC.FAULTY) if bots else [s for g in EC.FAULTY for s in (2 * g, 2 * g + 1)]


def _want(S, bit, slots):
    f = np.zeros(S, np.uint32)
    f[slots] = bit
    return f


def _flags_are(env, want, tag):
    got = env.error_flags()
    assert got.dtype == want.dtype and np.array_equal(got, want), f"{tag}: error flags {got.tolist()}, expected {want.tolist()}"


def _fresh_oracle(size, S, max_steps=2000, po=False):
    ref = oracle_py.OracleVecClient(S, 0, max_steps, [EC.MAPS[size]] * S, partial_obs=po, seed=SC.GAME_SEED)
    ref.reset()
    return ref


def _after_reset(A, ref, tag, env_steps=True, steps=10):
    """reset() on both sides clears every flag, and the whole handle then plays like the freshly reset oracle.
    (reset() leaves envSteps alone, JNIGridnetVecClient.java:179-211: they are compared where `ref` has run the same
    steps as A, not where it is a new oracle.)"""
    ref.reset()
    A.reset()
    _flags_are(A, _want(ref.S, 0, []), f"{tag} after reset()")
    assert not EC.errors(ref).any()
    assert_matches_oracle(A, ref, f"{tag} after reset()", states="even", env_steps=env_steps)
    for step in range(steps):
        A.random_policy(SEED, 100 + step)
        acts = A.actions.cpu().numpy()
        A.step()
        ref.step(acts)
        assert_matches_oracle(A, ref, f"{tag} step {step} after reset()", states="even", env_steps=env_steps)
    _flags_are(A, _want(ref.S, 0, []), f"{tag} {steps} steps after reset()")


# ------------------------------------------------------------------ MRTS_ERR_NEG_RESOURCES

NEG_STEPWISE = [(c, False) for c in EC.NEG_CASES] + [(((10, 10), None), True)]


@pytest.mark.parametrize("c,bots", NEG_STEPWISE, ids=[EC.case_id(c) + (" bots" if b else "") for c, b in NEG_STEPWISE])
def test_neg_resources_step_by_step(c, bots):
    """25 masked-random steps from the injection through step(), one launch per step, against the oracle at every
    step: the generic kernel (10x10 self-play; agent-vs-RandomBiasedAI envs), the specialised 16x16 (with at most 64
    units and crowded past them) and 8x8 instances, 32x32 partially observable with max_units = 256.  The flag is
    MRTS_ERR_NEG_RESOURCES on the faulty games from the step at which the oracle counts Java's print, not before, and
    nothing on any other slot; every game times out and resets inside the run, and the flag stays."""
    torch_gpu()
    size, seed = c
    po = size == (32, 32)
    faulty, _, fires_at = EC.neg_resources(size, crowd_seed=seed)
    states = EC.games(size, faulty)
    tag = f"neg_resources {EC.case_id(c)}{' bots' if bots else ''}"
    A = _env(size, states, MAX_STEPS, bots, po, EC.PO_MAX_UNITS if po else 0)
    ref = EC.oracle(size, states, MAX_STEPS, bots, po)
    S = ref.S
    bad = _bad_slots(bots)
    same(A.masks, ref.get_masks(0), "masks", f"{tag} injected")
    _flags_are(A, _want(S, 0, []), f"{tag} injected")
    seen = np.zeros(S, bool)
    dones = 0
    for step in range(STEPS):
        at = f"{tag} step {step}"
        A.random_policy(SEED, step)
        acts = A.actions.cpu().numpy()
        assert np.array_equal(acts, EC.masked_rows(ref, step)), f"{at}: policy rows"
        A.step()
        ref.step(acts)
        assert_matches_oracle(A, ref, at, states="all" if bots else "even", xy_free=True, env_steps=True)
        seen |= EC.errors(ref) > 0  # (a game that resets starts a new count; the kernels' flag is sticky)
        assert seen.nonzero()[0].tolist() == (bad if step + 1 >= fires_at else []), f"{at}: the oracle's prints {seen}"
        _flags_are(A, _want(S, EC.E_NEG_RESOURCES, bad if step + 1 >= fires_at else []), at)
        dones += int(ref.done.sum())
    assert dones >= S, f"{tag}: not every game reset inside a step"
    if not bots:
        _after_reset(A, ref, tag)
    A.close()
    ref.close()


def _same_with_flags(A, B, want, tag):
    """gpu_support.assert_same_outputs for two envs that hold flags: everything equal, and the flags the expected ones"""
    A.synchronize()
    B.synchronize()
    for name in ("obs", "masks", "actions", "source", "reward", "done"):
        same(getattr(A, name), getattr(B, name), name, tag)
    _flags_are(A, want, f"{tag} (multi-step)")
    _flags_are(B, want, f"{tag} (one launch per step)")
    assert np.array_equal(A._h.env_steps(), B._h.env_steps()), f"{tag}: env steps"
    for s in range(0, A._h.S, 2):
        assert np.array_equal(A.dump_state(s), B.dump_state(s)), f"{tag}: state of slot {s}"


def test_neg_resources_inside_a_fused_multi_step_launch():
    """rollout_fused on 16x16 with delta masks, launches of 3 and 22 steps: the production fails at step 10, in the
    middle of the second launch, whose header lives in LDS until the launch ends.  Against a twin that runs one launch
    per step, and against the oracle at both launch boundaries."""
    torch_gpu()
    size = (16, 16)
    faulty, _, fires_at = EC.neg_resources(size)
    assert 3 < fires_at < 25
    states = EC.games(size, faulty)
    M, O = _env(size, states), _env(size, states)
    O.set_multi_step(False)
    assert M.fused_multi_step and not O.fused_multi_step
    ref = EC.oracle(size, states)
    S, bad = ref.S, _bad_slots()
    for e in (M, O):
        e.random_policy(SEED, 0)
    k = 0
    for n in (3, 22):
        M.rollout_fused(SEED, k + 1, n)
        O.rollout_fused(SEED, k + 1, n)
        for t in range(k, k + n):
            ref.step(EC.masked_rows(ref, t))
        k += n
        tag = f"neg_resources fused, after the launch to step {k}"
        _same_with_flags(M, O, _want(S, EC.E_NEG_RESOURCES, bad if k >= fires_at else []), tag)
        assert (EC.errors(ref) > 0).nonzero()[0].tolist() == (bad if k >= fires_at else []), tag
        assert_matches_oracle(M, ref, tag, next_rows=EC.masked_rows(ref, k), states="even", xy_free=True, env_steps=True)
    for e in (M, O):
        e.close()
    ref.close()


def test_neg_resources_inside_a_uniform_multi_step_launch():
    """rollout_uniform on 8x8 (unmasked uniform rows drawn by the step kernel, no masks), launches of 3 and 22 steps,
    against the oracle taking the same rows.  (Java prints for other reasons too under unmasked rows, so the oracle's
    side shows the refusal by the state: the Base's production is gone and player 0 has neither paid nor gained a
    unit in that step.)"""
    torch_gpu()
    size = (8, 8)
    faulty, _, fires_at = EC.neg_resources(size)
    states = EC.games(size, faulty)
    M = _env(size, states)
    assert M.multi_step_capable
    ref = EC.oracle(size, states)
    S, H, W, C, K = M.dims
    bad = _bad_slots()
    k = 0
    for n in (3, 22):
        M.rollout_uniform(SEED, k, n)
        for t in range(k, k + n):
            rows = np.stack([oracle_py.policy_uniform(H, W, K, SEED, s, t) for s in range(S)])
            before = [dumps.parse(ref.dump(2 * g)) for g in EC.FAULTY]
            ref.step(rows)
            if t == fires_at - 1:
                for g, b in zip(EC.FAULTY, before):
                    a = dumps.parse(ref.dump(2 * g))
                    base = next(i for i, u in enumerate(b.units) if u[0] == 1 and u[1] == 0)
                    assert [r[1] for r in b.assign if r[0] == base] == [PRODUCE], "the production was under way"
                    assert not [r for r in a.assign if r[0] == base and r[1] == PRODUCE] and a.res[0] == b.res[0] == 0
                    assert (a.units[:, 1] == 0).sum() <= (b.units[:, 1] == 0).sum()
        k += n
        tag = f"neg_resources uniform, after the launch to step {k}"
        assert_matches_oracle(M, ref, tag, masks=None, next_rows=rows, states="even", xy_free=True, env_steps=True)
        _flags_are(M, _want(S, EC.E_NEG_RESOURCES, bad if k >= fires_at else []), tag)
    M.close()
    ref.close()


def _client(size, states):
    """tests.JNIGridnetVecClient's mirror (the host-pointer calls) with these games"""
    from microrts_amd import JNIGridnetVecClient

    n = len(states)
    vc = JNIGridnetVecClient(2 * n, 0, 2000, None, "", [EC.MAPS[size]] * (2 * n), seed=SC.GAME_SEED)
    vc.reset()
    for g, j in enumerate(states):
        vc.setGameStateJSON(2 * g, j)
    return vc


def test_neg_resources_does_not_fail_gamestep():
    """Java only prints: gameStep goes on through the step that raises the flag, with the oracle's responses."""
    torch_gpu()
    size = (10, 10)
    faulty, _, fires_at = EC.neg_resources(size)
    states = EC.games(size, faulty)
    vc = _client(size, states)
    ref = EC.oracle(size, states)
    for step in range(fires_at + 2):
        acts = EC.masked_rows(ref, step)
        r = vc.gameStep(acts)
        ref.step(acts)
        assert np.array_equal(r.observation, ref.obs) and np.array_equal(r.reward[:, 0], ref.reward), step
    assert np.array_equal(vc.error_flags(), _want(ref.S, EC.E_NEG_RESOURCES, _bad_slots()))
    vc.close()
    ref.close()


# ------------------------------------------------------------------ MRTS_ERR_ADDUNIT


@pytest.mark.parametrize("c", EC.ADDUNIT_CASES, ids=EC.case_id)
def test_addunit_leaves_the_twin(c):
    """The firing step (all-zero rows: a pending PRODUCE reserves a cell and resources where the twin's NONE does not,
    and zero rows issue nothing that could tell) and 20 masked-random steps more: the faulty games equal the oracle
    on the NONE twin, the controls the oracle.  Generic kernel (12x12) and specialised 16x16, with at most 64 units
    (one unit per lane) and crowded past them (the LDS ready list)."""
    torch_gpu()
    size, seed = c
    faulty, twin, fires_at = EC.addunit(size, crowd_seed=seed)
    assert fires_at == 1
    tag = f"addunit {EC.case_id(c)}"
    A = _env(size, EC.games(size, faulty))
    ref = EC.oracle(size, EC.games(size, twin))
    want = _want(ref.S, EC.E_ADDUNIT, _bad_slots())
    _flags_are(A, _want(ref.S, 0, []), f"{tag} injected")
    A.actions.zero_()
    A.step()
    ref.step(EC.zero_rows(ref))
    assert_matches_oracle(A, ref, f"{tag} firing step", states="even", xy_free=True, env_steps=True)
    _flags_are(A, want, f"{tag} firing step")
    for step in range(20):
        A.random_policy(SEED, step)
        acts = A.actions.cpu().numpy()
        assert np.array_equal(acts, EC.masked_rows(ref, step)), f"{tag} step {step}: policy rows"
        A.step()
        ref.step(acts)
        assert_matches_oracle(A, ref, f"{tag} step {step} after firing", states="even", xy_free=True, env_steps=True)
    _flags_are(A, want, f"{tag} at the end")
    assert not EC.errors(ref).any()
    A.close()
    ref.close()


def _step_fails(vc, acts, code, text):
    with pytest.raises(RuntimeError, match=f"mrts error {code}: {text}"):
        vc.gameStep(acts)


@pytest.mark.parametrize("scenario", ["addunit", "collision"])
def test_two_units_in_a_cell_fail_gamestep_until_reset(scenario):
    """-EFAULT with checkFlagsAfter's words from the firing gameStep, again from the next one (the flag is sticky),
    and none after reset()."""
    torch_gpu()
    size = (16, 16)
    faulty, _, _ = EC.addunit(size) if scenario == "addunit" else EC.collision(size)
    vc = _client(size, EC.games(size, faulty))
    zeros = np.zeros((vc.num_slots, 256, 7), np.int32)
    bit = EC.E_ADDUNIT if scenario == "addunit" else EC.E_MOVE_COLLISION
    for _ in range(2):
        _step_fails(vc, zeros, EFAULT, "two units in one position")
        assert np.array_equal(vc.error_flags(), _want(vc.num_slots, bit, _bad_slots()))
    ref = _fresh_oracle(size, vc.num_slots)
    r = vc.reset()
    assert not vc.error_flags().any() and np.array_equal(r.observation, ref.obs)
    acts = EC.masked_rows(ref, 0)
    r = vc.gameStep(acts)
    ref.step(acts)
    assert np.array_equal(r.observation, ref.obs) and not vc.error_flags().any()
    vc.close()
    ref.close()


# ------------------------------------------------------------------ MRTS_ERR_MOVE_COLLISION


@pytest.mark.parametrize("size", EC.COLLISION_SIZES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_collision_stays_in_its_game(size):
    """The control games equal an oracle of the controls alone at the firing step and for 10 masked-random steps
    after it, while the faulty games (two units on one cell, stepped on) are not looked at; then reset(), and the
    whole handle equals a freshly reset oracle for 10 steps: nothing the fault wrote survives."""
    torch_gpu()
    faulty, _, fires_at = EC.collision(size)
    assert fires_at == 1
    tag = f"collision {size[1]}x{size[0]}"
    states = EC.games(size, faulty)
    controls = [g for g in range(EC.GAMES) if g not in EC.FAULTY]
    slots = [s for g in controls for s in (2 * g, 2 * g + 1)]
    A = _env(size, states)
    ref = EC.oracle(size, [states[g] for g in controls])
    want = _want(A._h.S, EC.E_MOVE_COLLISION, _bad_slots())
    A.actions.zero_()
    A.step()
    ref.step(EC.zero_rows(ref))
    assert_matches_oracle(A, ref, f"{tag} firing step", slots=slots, states="even", xy_free=True, env_steps=True)
    _flags_are(A, want, f"{tag} firing step")
    for step in range(10):
        A.random_policy(SEED, step)
        acts = A.actions.cpu().numpy()
        m = ref.get_masks(0)
        rows = np.stack([oracle_py.policy(m[i], SEED, s, step, 0) for i, s in enumerate(slots)])
        assert np.array_equal(acts[slots], rows), f"{tag} step {step}: the controls' policy rows"
        A.step()
        ref.step(rows)
        assert_matches_oracle(A, ref, f"{tag} step {step} after firing", slots=slots, states="even", xy_free=True,
                              env_steps=True)
        assert np.array_equal(A.error_flags()[slots], np.zeros(len(slots), np.uint32)), f"{tag} step {step}: the controls' flags"
    assert (A.error_flags()[_bad_slots()] & EC.E_MOVE_COLLISION).all()
    fresh = _fresh_oracle(size, A._h.S)
    _after_reset(A, fresh, tag, env_steps=False)
    A.close()
    ref.close()
    fresh.close()


# ------------------------------------------------------------------ MRTS_ERR_CAPACITY


def _host_handle(size, states, max_units):
    """The host-pointer calls on a handle with max_units (the vec-client mirror has no such argument): a bare handle,
    reset through mrts_reset, states injected -> (handle, step(actions) -> (return code, mrts_last_error()))"""
    from microrts_amd import UnitTypeTable, _lib
    from microrts_amd.vec_client import _Handle, _resolve

    n = len(states)
    h = _Handle(2 * n, 0, 2000, [_resolve("", EC.MAPS[size])] * (2 * n), None, UnitTypeTable(), False, 0, SC.GAME_SEED, 0,
                max_units=max_units)
    resp = _lib.MrtsResponses()
    assert h.L.mrts_reset(h.h, None, ctypes.byref(resp)) == 0
    for g, j in enumerate(states):
        if j is not None:
            h.set_state_json(2 * g, j)

    def step(actions):
        a = np.ascontiguousarray(actions, np.int32)
        rc = h.L.mrts_step(h.h, a.ctypes.data_as(ctypes.c_void_p), None, ctypes.byref(resp))
        return rc, h.L.mrts_last_error().decode()

    def reset():
        return h.L.mrts_reset(h.h, None, ctypes.byref(resp))

    return h, step, reset


@pytest.mark.parametrize("producers", [64, 66])
def test_capacity(producers):
    """16x16 with max_units = 68 (132 unit slots), 68 units, `producers` Bases completing PRODUCE Worker in one cycle.
    64: every birth lands, nu reaches the capacity exactly, no flag, the state is the oracle's.  66 (more than 64
    ready assignments: cycle()'s repeated minimum search): the first 64 land in list order, MRTS_ERR_CAPACITY, the
    state is the oracle's of the twin whose last two producers held NONE.  The games are not stepped on ("env must be
    reset"); reset() clears the flag.  mrts_step answers 0 and -ENOSPC."""
    torch_gpu()
    size, M = EC.CAPACITY_SIZE, EC.CAPACITY_UNITS
    faulty, twin, _ = EC.capacity(producers)
    full = producers > 64
    tag = f"capacity {producers}"
    states = EC.games(size, faulty, max_units=M)
    A = _env(size, states, max_units=M)
    ref = EC.oracle(size, EC.games(size, twin if full else faulty, max_units=M))
    want = _want(ref.S, EC.E_CAPACITY, _bad_slots() if full else [])
    A.actions.zero_()
    A.step()
    ref.step(EC.zero_rows(ref))
    assert_matches_oracle(A, ref, tag, states="even", xy_free=True, env_steps=True)
    _flags_are(A, want, tag)
    for g in EC.FAULTY:
        st = dumps.parse(A.dump_state(2 * g))
        assert len(st.units) == M + 64 == M + max(64, M // 4) and st.res == (100 - 64, 5), f"{tag}: 64 Workers, 64 costs paid"
    _after_reset(A, ref, tag, steps=3)
    A.close()
    ref.close()
    h, step, reset = _host_handle(size, states, M)
    rc, msg = step(np.zeros((h.S, 256, 7), np.int32))
    assert (rc, msg) == ((ENOSPC, "unit capacity exhausted") if full else (0, msg)), (rc, msg)
    assert np.array_equal(h.error_flags(), want)
    assert reset() == 0 and not h.error_flags().any()
    h.close()


def test_return_code_order():
    """One game with MRTS_ERR_CAPACITY and another with MRTS_ERR_PRODUCE_TYPE (a produce type outside the table in
    a row for its idle Base) in one step: mrts_step answers checkFlagsAfter's first test, -EINVAL."""
    torch_gpu()
    size, M = EC.CAPACITY_SIZE, EC.CAPACITY_UNITS
    faulty, _, _ = EC.capacity(66)
    g_cap, g_type = EC.FAULTY
    h, step, _ = _host_handle(size, [faulty if g == g_cap else None for g in range(EC.GAMES)], M)
    st = dumps.parse(h.dump(2 * g_type))
    base = next(u for u in st.units if u[0] == 1 and u[1] == 0)
    acts = np.zeros((h.S, 256, 7), np.int32)
    acts[2 * g_type, base[3] * 16 + base[2]] = [PRODUCE, 0, 0, 0, RIGHT, 7, 0]
    rc, msg = step(acts)
    assert rc == EINVAL and msg.startswith("decoded produce type out of range"), (rc, msg)
    want = _want(h.S, EC.E_CAPACITY, [2 * g_cap, 2 * g_cap + 1])
    want[[2 * g_type, 2 * g_type + 1]] = EC.E_PRODUCE_TYPE
    assert np.array_equal(h.error_flags(), want), h.error_flags()
    h.close()


# ------------------------------------------------------------------ MRTS_ERR_OLDER_CONFLICT


@pytest.mark.parametrize("generic", [False, True], ids=["chosen instance", "generic"])
def test_older_conflict_through_trace_step(generic):
    """The hand-written trace of tests/error_cases.py on game 0 of a forward model, the same trace without the
    conflicting action on game 1: every entry's state equals the oracle's lenient replay, the refused entry reports
    no issued action, Light 33 holds NONE with parameter -1, and the flag is MRTS_ERR_OLDER_CONFLICT on game 0 alone."""
    torch_gpu()
    from microrts_amd import ForwardModel

    mp = os.path.join(SC.ROOT, EC.OLDER_MAP)
    clean_text = EC.OLDER_CONFLICT_TRACE.replace("A 1\na 33 1 1 0 0 -1\n", "A 0\n")
    texts = [EC.OLDER_CONFLICT_TRACE, clean_text]
    entries = [parse(t) for t in texts]
    want, issued, errs = oracle_py.trace_dumps(mp, texts[0], lenient=True)
    want_clean, issued_clean = oracle_py.trace_dumps(mp, texts[1])
    assert errs.tolist() == [0, 0, 1, 1, 1] and issued.tolist() == [1, 1, 0, 0, 0] and issued_clean.tolist() == [1, 1, 0, 0, 0]
    fm = ForwardModel(2, [mp, mp], policies=("PassiveAI", "PassiveAI"))
    n = len(entries[0])
    for k in range(n):
        rows = [issue_rows(e[k - 1][3]) if k else [] for e in entries]
        pairs = np.full((2, 1, 8), -1, dtype=np.int32)
        for g, r in enumerate(rows):
            if r:
                pairs[g, :len(r)] = np.array(r, dtype=np.int32)
        flags = fm.trace_step(pairs, [e[k][0] for e in entries], generic=generic)  # returns: the call's code was 0
        tag = f"older conflict entry {k}"
        assert not (flags & ~TRACE_ISSUED).any(), f"{tag}: {flags}"
        if k:
            assert (flags & TRACE_ISSUED).tolist() == [issued[k - 1], issued_clean[k - 1]], f"{tag}: issued {flags}"
        for g, ref in enumerate((want, want_clean)):
            d = fm.dump_state(g)
            check_vs_trace(d, entries[g][k], f"{tag} game {g}")
            assert np.array_equal(d, ref[k]), f"{tag} game {g}: {dumps.difference(d, ref[k])}"
        _flags = fm.error_flags()
        assert _flags.tolist() == [EC.E_OLDER_CONFLICT if k > EC.OLDER_ENTRY else 0, 0], f"{tag}: error flags {_flags}"
        if k == EC.OLDER_ENTRY + 1:
            a, _ = dumps.assignment_of(fm.dump_state(0), 1)
            assert a[1] == NONE and a[2] == -1, f"{tag}: Light 33 holds {a.tolist()}"
    fm.close()
