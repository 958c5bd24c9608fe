"""The outputs on every map shape, from injected mid-game states, bit-exact against the CPU oracle.

tests/test_gpu_traces.py pins the state engine on all 17 map sizes of the reference traces; the outputs
(observation planes, partially observable views, masks, source bits, rewards, dones, action decode, the
in-step auto-reset) were compared with the oracle step by step only on square maps of at most 32x32 and
only from start positions.  Here every size (4x4 .. 128x128; 9x8, 16x8, 14x12, 16x12, 15x14, 128x96,
96x128, 128x112 among them) is stepped from the games of tests.state_cases: states the recorded games
pass through and crowded copies holding all seven unit types, both owners and, from 144 cells up, more
than 64 units.  max_steps lies below the stepped horizon, so every game also resets inside a step.

* handle A (delta masks, delta observations, source bits) against the oracle: masks and source bits
  after the injection; on every step the policy kernel's rows (first 8 slots), observations, rewards,
  dones and masks; the state dump every 5th step;
* handle B (full mask and observation writes, no source bits) takes the same actions, on odd steps as
  Java rows [pos, 7 components] in ascending order through step_rows, and must equal A after every step;
* handle C takes the same steps through step_fused and must equal A, action rows included;
* reversed Java rows: PlayerAction.fromVectorAction gives the rows of one player priority in list order
  (ResourceUsage.consistentWith: a cell or the resources a row claims are refused to every later row,
  tests/test_kats.py A.4), so rows in another order are another step than the grid's and cannot equal A.
  They are compared with what defines them, the oracle's step_rows over the same list: B and the oracle
  take the states once more and step REVERSED_STEPS times on reversed rows;
* the one-hot encoder on A's observation half-way to the reset and on its last one, against the numpy
  restatement of tests.gpu_checks.
"""
import json

import numpy as np
import pytest

from tests import oracle_py, policy_head_ref
from tests import state_cases as SC
from tests.gpu_checks import encode_obs_np
from tests.gpu_support import assert_matches_oracle, same, torch_gpu

pytestmark = pytest.mark.gpu

SEED = SC.SEED
REVERSED_STEPS = 4


def _inject(handle, states, stride):
    for g, j in enumerate(states):
        handle.set_state_json(stride * g, j)


def _check_injected(A, ref, tag):
    """After the injection, before any step: A's masks (both players' views in self-play) and source bits."""
    A.get_masks()
    m = ref.get_masks(0)
    same(A.masks, m, "masks", f"{tag} injected")
    same(A.source, policy_head_ref.source_bits(m.reshape(ref.S, -1, ref.K)), "source bits", f"{tag} injected")
    return m


def _check_onehot(A, po, tag):
    got = A.onehot_obs()
    want = encode_obs_np(A.obs.cpu().numpy(), 7)
    assert got.shape == want.shape and got.shape[-1] == (33 if po else 29)
    same(got, want, "one-hot observation", tag)


def _make(c, po, bots, **kw):
    from microrts_amd import DeviceVecEnv

    n = len(c["states"])
    if bots:
        return DeviceVecEnv(0, n, c["max_steps"], c["maps"], ai2s=["RandomBiasedAI"] * n, seed=SC.GAME_SEED, partial_obs=po,
                            max_units=c["max_units"], **kw)
    return DeviceVecEnv(2 * n, 0, c["max_steps"], c["maps"], seed=SC.GAME_SEED, partial_obs=po, max_units=c["max_units"], **kw)


def _oracle(c, po, bots):
    n = len(c["states"])
    if bots:
        return oracle_py.OracleVecClient(0, n, c["max_steps"], c["maps"], partial_obs=po, seed=SC.GAME_SEED,
                                         bot_kinds=[oracle_py.BOT_RANDOM_BIASED] * n)
    return oracle_py.OracleVecClient(2 * n, 0, c["max_steps"], c["maps"], partial_obs=po, seed=SC.GAME_SEED)


def _run(c, po, bots=False):
    torch = torch_gpu()
    tag = f"{c['size'][1]}x{c['size'][0]}{' po' if po else ''}{' bots' if bots else ''}"
    stride = 1 if bots else 2
    every = "all" if bots else "even"  # the slots whose state is compared: one per game
    players = c.get("players") if bots else None
    A = _make(c, po, bots)
    twins = [] if bots else [_make(c, po, bots, mask_delta=False, obs_delta=False, source_bits=False), _make(c, po, bots)]
    ref = _oracle(c, po, bots)
    S, HW = ref.S, ref.H * ref.W
    assert A.dims == (S, ref.H, ref.W, ref.C, ref.K)
    for e in [A] + twins:
        if players is not None:
            e.players.copy_(torch.as_tensor(players, dtype=torch.int32))
        e.reset()
        _inject(e, c["states"], stride)
    ref.reset(players)
    _inject(ref, c["states"], stride)
    _check_injected(A, ref, tag)
    for e in twins:
        e.get_masks()
    if twins:
        B, C = twins
        C.random_policy(SEED, 0)
        pos = torch.arange(HW, dtype=torch.int32, device=A.device).reshape(1, HW, 1).expand(S, HW, 1)
    dones = 0
    for step in range(c["steps"]):
        at = f"{tag} step {step}"
        A.random_policy(SEED, step)
        acts = A.actions.cpu().numpy()
        m = ref.get_masks(0)
        for s in range(min(S, 8)):
            assert np.array_equal(acts[s], oracle_py.policy(m[s], SEED, s, step, 0)), f"{at}: policy rows of slot {s}"
        if twins:
            same(C.actions, A.actions, "C's fused policy rows", at)
            if step % 2:
                B.step_rows(torch.cat([pos, A.actions], dim=2).contiguous())
            else:
                B.step(A.actions)
            C.step_fused(SEED, step + 1)
        A.step()
        ref.step(acts, players)  # raises what Java would throw
        dones += int(ref.done.sum())
        assert_matches_oracle(A, ref, at, states=every if step % 5 == 4 else None, xy_free=True)
        for name, e in zip(("B", "C"), twins):
            for what in ("obs", "masks", "reward", "done"):
                same(getattr(e, what), getattr(A, what), f"{name}.{what} vs A", at)
        if step == c["max_steps"] // 2:  # the crowd is still on the map
            _check_onehot(A, po, at)
    assert dones >= S, f"{tag}: not every game reset inside a step ({dones} dones, {S} slots)"
    _check_onehot(A, po, tag)
    if twins:
        A.random_policy(SEED, c["steps"])
        same(C.actions, A.actions, "C's fused policy rows", f"{tag} after the last step")
        # reversed Java rows, against the oracle's step_rows from the same states
        _inject(B, c["states"], stride)
        _inject(ref, c["states"], stride)
        B.get_masks()
        same(B.masks, ref.get_masks(0), "masks", f"{tag} injected again")
        for k in range(REVERSED_STEPS):
            at = f"{tag} reversed rows step {k}"
            B.random_policy(SEED, 1000 + k)
            rows = torch.cat([pos, B.actions], dim=2).flip(1).contiguous()
            B.step_rows(rows)
            ref.step_rows(rows.cpu().numpy())
            assert_matches_oracle(B, ref, at, states=every if k == REVERSED_STEPS - 1 else None, xy_free=True)
    for name, e in zip("ABC", [A] + twins):
        assert not e.error_flags().any(), f"{tag}: error flags of {name}: {e.error_flags()}"
        e.close()
    ref.close()


def _id(size):
    return f"{size[1]}x{size[0]}"


@pytest.mark.parametrize("po", [False, True], ids=["full", "po"])
@pytest.mark.parametrize("size", SC.SIZES, ids=_id)
def test_outputs_on_every_shape(size, po):
    _run(SC.case(size), po)


@pytest.mark.parametrize("size", SC.BOT_SIZES, ids=_id)
def test_outputs_against_bots(size):
    """Agent-vs-RandomBiasedAI envs, players alternating 0 / 1, full observability, on 9x8, 14x12 and
    128x96: the same states injected into the bot envs of both sides (the opponents' random streams are
    kept), compared with the oracle in handle A's form."""
    _run(SC.bot_case(size), False, bots=True)


def test_a_shifted_unit_is_noticed():
    """The comparison is not vacuous: on 128x96, one crowd unit moved by one cell in the oracle's copy
    alone makes the mask comparison fail before any step."""
    torch_gpu()
    c = SC.case((96, 128))
    g = c["crowded"].index(True)
    d = json.loads(c["states"][g])
    pgs = d["pgs"]
    W = pgs["width"]
    occupied = {(u["x"], u["y"]) for u in pgs["units"]}
    for u in pgs["units"][c["trace_units"][g]:]:
        x, y = u["x"] + 1, u["y"]
        if u["player"] >= 0 and x < W and pgs["terrain"][y * W + x] == "0" and (x, y) not in occupied:
            u["x"] = x
            break
    else:
        raise AssertionError("no crowd unit with a free cell to its right")
    shifted = list(c["states"])
    shifted[g] = json.dumps(d, separators=(",", ":"))
    A = _make(c, False, False)
    ref = _oracle(c, False, False)
    A.reset()
    ref.reset()
    _inject(A, c["states"], 2)
    _inject(ref, shifted, 2)
    with pytest.raises(AssertionError, match="masks differs"):
        _check_injected(A, ref, "shifted")
    _inject(ref, c["states"], 2)
    _check_injected(A, ref, "unshifted")
    A.close()
    ref.close()
