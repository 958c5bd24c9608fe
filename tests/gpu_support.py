"""What a GPU test needs before and after it runs kernels: the GPU guard, the pointer helper and the three
comparators every output comparison goes through.  Test infrastructure only (a plain helper module: its asserts
carry their own messages, pytest rewrites none of them).

* same(got, want, name, tag)            one tensor against an array or a tensor
* assert_matches_oracle(env, ref, tag)  a device env against the CPU oracle
* assert_same_outputs(A, B, tag)        two device envs against each other (or against a Record: one env's
                                        outputs as they stood at an earlier moment)

tests/test_gpu_support_cpu.py shows on stand-ins that each of them fails on a difference in each output."""
import ctypes

import numpy as np

from tests import dumps


def torch_gpu():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def same(got, want, name, tag, slots=None):
    """got (tensor) == want (numpy array or tensor), shape and dtype included, compared where got lives.
    slots: the slot behind each index of the first axis, for the message."""
    import torch

    w = want if isinstance(want, torch.Tensor) else torch.as_tensor(want, device=got.device)
    if got.shape == w.shape and got.dtype == w.dtype and torch.equal(got, w):
        return
    g, h = got.cpu().numpy(), w.cpu().numpy()
    assert g.shape == h.shape and g.dtype == h.dtype, f"{tag}: {name} {g.dtype}{g.shape} vs {h.dtype}{h.shape}"
    bad = np.argwhere(g != h)
    first = bad[0].tolist()
    slot = "" if slots is None else f" (slot {int(slots[first[0]])})"
    raise AssertionError(f"{tag}: {name} differs at {len(bad)} places, first {first}{slot}: "
                         f"gpu {g[tuple(bad[0])]} ref {h[tuple(bad[0])]}")


def _same_state(a, b, what, xy_free=False):
    if xy_free:
        a, b = dumps.xy_free(a), dumps.xy_free(b)
    assert np.array_equal(a, b), f"{what} differs {dumps.difference(a, b)}"


def assert_matches_oracle(env, ref, tag, slots=None, masks=0, next_rows=None, rewards="all", states="all", xy_free=False,
                          env_steps=False):
    """The device env's outputs equal the oracle's: observations, rewards and dones always, the rest as asked.

    slots      None: env slot i against oracle slot i, every slot.  A list: env slot slots[i] against oracle slot i
               (an oracle that replays picked games); the env's other slots are not looked at.
    masks      the player whose ref.get_masks(player) the mask buffer must equal, or None (a handle without masks).
    next_rows  the action rows the env must hold for the next step, one [H*W][7] per compared slot, or for the
               first len(next_rows) of them; None: not compared.
    rewards    "all": ref.reward / ref.done as they are; "first": their column 0 (an oracle with several reward
               functions against a handle with the first one); None: not compared (a handle with a Responses ring).
    states     "all": every compared slot's state dump; "even": every other one (both slots of a self-play game
               dump the same game); None: none.  xy_free: through dumps.xy_free (states injected as JSON).
    env_steps  also every compared slot's envSteps counter."""
    import torch

    env.synchronize()
    n = ref.S
    sl = list(range(n)) if slots is None else [int(s) for s in slots]
    assert len(sl) == n, f"{tag}: {len(sl)} slots picked for an oracle of {n}"
    if slots is None:
        pick = lambda t: t  # noqa: E731
    else:
        idx = torch.as_tensor(sl, dtype=torch.long, device=env.obs.device)
        pick = lambda t: t[idx]  # noqa: E731
    same(pick(env.obs), ref.obs, "obs", tag, sl)
    if rewards is not None:
        assert rewards in ("all", "first"), rewards
        col = (lambda a: a) if rewards == "all" else (lambda a: np.ascontiguousarray(a[:, 0]))  # noqa: E731
        same(pick(env.reward), col(ref.reward), "reward", tag, sl)
        same(pick(env.done), col(ref.done), "done", tag, sl)
    if masks is not None:
        same(pick(env.masks), ref.get_masks(masks), "masks", tag, sl)
    if next_rows is not None:
        got = pick(env.actions)[:len(next_rows)]
        want = np.asarray(next_rows)
        assert want.dtype.kind == "i" and want.size == got.numel(), f"{tag}: next action rows {want.dtype}{want.shape}"
        same(got, want.astype(np.int32).reshape(tuple(got.shape)), "next action rows", tag, sl)
    if states is not None:
        assert states in ("all", "even"), states
        for i in range(0, n, 1 if states == "all" else 2):
            _same_state(env.dump_state(sl[i]), ref.dump(i), f"{tag}: state of slot {sl[i]}", xy_free)
    if env_steps:
        got = env._h.env_steps()
        for i, s in enumerate(sl):
            assert int(got[s]) == ref.env_steps(i), f"{tag}: env steps of slot {s}: gpu {int(got[s])} ref {ref.env_steps(i)}"


class Record:
    """Everything assert_same_outputs compares, copied out of a device env as it stands: a later
    assert_same_outputs(env, record, tag) holds that env (or another) to this moment."""

    def __init__(self, env):
        env.synchronize()
        for name in ("obs", "masks", "actions", "source", "reward", "done"):
            t = getattr(env, name)
            setattr(self, name, None if t is None else t.clone())
        self._flags = env.error_flags().copy()
        self._steps = env._h.env_steps().copy()
        self.S = env._h.S
        self._states = {s: env.dump_state(s).copy() for s in range(0, self.S, 2)}
        self._h = self

    def synchronize(self):
        pass

    def error_flags(self):
        return self._flags

    def env_steps(self):
        return self._steps

    def dump_state(self, s):
        return self._states[s]


def assert_same_outputs(A, B, tag):
    """Two device envs hold the same thing: observations, masks, action rows, source bits, rewards, dones, error
    flags (equal, and none set), env steps and every other slot's state dump."""
    A.synchronize()
    B.synchronize()
    for name in ("obs", "masks", "actions", "source", "reward", "done"):
        a, b = getattr(A, name), getattr(B, name)
        assert a is not None and b is not None, f"{tag}: a handle without {name}"
        same(a, b, name, tag)
    fa, fb = A.error_flags(), B.error_flags()
    assert np.array_equal(fa, fb), f"{tag}: error flags differ: {fa} vs {fb}"
    assert not fa.any(), f"{tag}: error flags set: {fa}"
    ea, eb = A._h.env_steps(), B._h.env_steps()
    assert np.array_equal(ea, eb), f"{tag}: env steps differ, first at slot {int(np.argmax(ea != eb))}: {ea} vs {eb}"
    for s in range(0, A._h.S, 2):
        _same_state(A.dump_state(s), B.dump_state(s), f"{tag}: state of slot {s}")
