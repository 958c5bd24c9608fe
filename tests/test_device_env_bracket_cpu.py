"""DeviceVecEnv's one bracket around the entry points that write `obs` (DeviceVecEnv._write), on a stand-in: CPU
tensors, no handle, and a library object that records the calls it gets.  The invalidate calls fire exactly when a
version counter moved, in the order policy, obs, entry; the stamps and the ring bookkeeping are taken after the call,
and not at all when the call returns an error.  CPU only, no built library."""
import types

import pytest
import torch

from microrts_amd import DeviceVecEnv, _lib

STREAM = types.SimpleNamespace(cuda_stream=0)  # an explicit stream: torch's current HIP stream needs a GPU


class RecordingLibrary:
    """Every mrts_* attribute is a function that records (name, args, the env's stamps when it was called) and
    returns 0, or -22 for the names in `fail`."""

    def __init__(self):
        self.calls, self.fail, self.env = [], set(), None

    def __getattr__(self, name):
        if not name.startswith("mrts_"):
            raise AttributeError(name)

        def call(*args):
            e = self.env
            self.calls.append((name, args, (e._obs_version, e._policy_out, e._policy_version, e._ring_last)))
            return -22 if name in self.fail else 0

        return call

    def mrts_last_error(self):
        return b"refused by the stand-in"

    def names(self):
        out = [c[0] for c in self.calls]
        self.calls.clear()
        return out


@pytest.fixture
def env(monkeypatch):
    L = RecordingLibrary()
    monkeypatch.setattr(_lib, "_lib", L)  # _lib.check reads the error text from the loaded library
    e = DeviceVecEnv.__new__(DeviceVecEnv)
    S, H, W, C, K = 2, 4, 4, 6, 79
    e._h = types.SimpleNamespace(L=L, h="handle", S=S, H=H, W=W, C=C, K=K, R=1)
    e.torch, e.device = torch, torch.device("cpu")
    e.obs = torch.zeros((S, C, H, W), dtype=torch.int32)
    e._reward, e._done = torch.zeros(S, dtype=torch.float64), torch.zeros(S, dtype=torch.uint8)
    e.masks = torch.zeros((S, H, W, K), dtype=torch.uint8)
    e.actions, e.players = torch.zeros((S, H * W, 7), dtype=torch.int32), torch.zeros(S, dtype=torch.int32)
    e.source, e.mask_player = None, 0
    e.step_rewards = e.step_dones = e._ring_last = None
    e._policy_out, e._policy_version, e._obs_version, e._ptr_cache = None, -1, -1, None
    L.env = e
    return e


FORMS = {
    "rollout_fused": (lambda e, n: e.rollout_fused(7, 3, n, stream=STREAM), "mrts_rollout_fused_dev", True),
    "rollout_uniform": (lambda e, n: e.rollout_uniform(7, 3, n, stream=STREAM), "mrts_rollout_uniform_dev", False),
    "rollout_fused_records": (lambda e, n: e.rollout_fused_records(7, 3, n, e.obs, stream=STREAM),
                              "mrts_rollout_fused_records_dev", True),
    "rollout_uniform_exchange": (lambda e, n: e.rollout_uniform_exchange(7, 3, n, (e.obs, e.obs), e.obs, stream=STREAM),
                                 "mrts_rollout_uniform_exchange_dev", False),
}


@pytest.mark.parametrize("form", list(FORMS))
def test_invalidates_fire_exactly_when_a_version_moved(env, form):
    run, entry, policy = FORMS[form]
    L = env._h.L
    run(env, 1)
    assert L.names() == ["mrts_obs_invalidate", entry]  # a new env: obs was never written by the library
    run(env, 1)
    assert L.names() == [entry]
    env.obs.add_(1)
    run(env, 1)
    assert L.names() == ["mrts_obs_invalidate", entry]
    env.actions.add_(1)  # someone else's rows
    run(env, 1)
    assert L.names() == (["mrts_policy_invalidate", entry] if policy else [entry])
    env.actions.add_(1)
    env.obs.add_(1)
    run(env, 1)
    assert L.names() == (["mrts_policy_invalidate"] if policy else []) + ["mrts_obs_invalidate", entry]
    run(env, 1)
    assert L.names() == [entry]
    # a tensor put in actions' place is not the one the library's last policy output is in: nothing to invalidate
    env.actions = env.actions.clone()
    run(env, 1)
    assert L.names() == [entry]


@pytest.mark.parametrize("form", list(FORMS))
def test_stamps_are_taken_after_the_call(env, form):
    run, entry, policy = FORMS[form]
    L = env._h.L
    env.step_rewards, env.step_dones = torch.zeros((4, 2)), torch.zeros((4, 2))
    env.obs.add_(1)
    env.actions.add_(1)
    run(env, 3)
    name, args, (obs_v, pol_out, pol_v, ring) = L.calls[-1]
    assert name == entry and (obs_v, pol_out, pol_v, ring) == (-1, None, -1, None)  # nothing stamped when it ran
    assert env._obs_version == env.obs._version == 1 and env._ring_last == 2
    if policy:
        assert env._policy_out is env.actions and env._policy_version == env.actions._version == 1
    else:
        assert env._policy_out is None and env._policy_version == -1
    # the call got the handle, the cached pointers of actions, players, obs, reward, done and the stream
    assert args[0] == "handle" and args[-1].value in (0, None)
    assert [p.value for p in args[1:6]] == [t.data_ptr() for t in (env.actions, env.players, env.obs, env._reward, env._done)]
    first = args[1:6]
    L.calls.clear()
    run(env, 0)  # no step: the ring's last step stays
    assert env._ring_last == 2
    assert all(a is b for a, b in zip(L.calls[-1][1][1:6], first)), "the pointers were converted again"
    env.step_fused(7, 9, stream=STREAM)  # a single step writes the plain reward / done
    assert env._ring_last is None and env._policy_out is env.actions


@pytest.mark.parametrize("form", list(FORMS))
def test_a_refused_call_leaves_the_stamps_and_the_ring(env, form):
    run, entry, policy = FORMS[form]
    L = env._h.L
    env.step_rewards, env.step_dones = torch.zeros((4, 2)), torch.zeros((4, 2))
    env.step_fused(7, 1, stream=STREAM)
    run(env, 2)
    assert env._ring_last == 1
    before = (env._obs_version, env._policy_out, env._policy_version)
    env.obs.add_(1)
    env.actions.add_(1)
    L.calls.clear()
    L.fail = {entry}
    with pytest.raises(RuntimeError, match="mrts error -22: refused by the stand-in"):
        run(env, 4)
    assert L.names()[-1] == entry
    assert (env._obs_version, env._policy_out, env._policy_version) == before and env._ring_last == 1
    assert env._obs_version != env.obs._version and env._policy_version != env.actions._version
    L.fail = set()
    run(env, 4)  # the guards fire again: nothing was stamped
    assert L.names() == (["mrts_policy_invalidate"] if policy else []) + ["mrts_obs_invalidate", entry]
    assert env._ring_last == 3


def recorded_calls(env):
    """(name, arguments with each pointer as its address) of the entry-point calls of all eleven bracketed methods, the
    optional arguments of step / step_uniform included"""
    L = env._h.L
    rows = torch.zeros((2, 3, 8), dtype=torch.int32)
    other = torch.zeros_like(env.actions)
    send, recv = (torch.zeros(4), torch.zeros(5)), torch.zeros(6)
    for call in (lambda: env.reset(stream=STREAM), lambda: env.step(stream=STREAM),
                 lambda: env.step(actions=other, masks=False, stream=STREAM), lambda: env.step(masks=False, stream=STREAM),
                 lambda: env.step_uniform(7, 1, stream=STREAM), lambda: env.step_uniform(7, 2, masks=True, stream=STREAM),
                 lambda: env.step_rows(rows, stream=STREAM), lambda: env.step_fused(7, 3, stream=STREAM),
                 lambda: env.rollout_fused(7, 4, 2, stream=STREAM), lambda: env.rollout_fused_exchange(7, 5, 2, send, recv, stream=STREAM),
                 lambda: env.rollout_fused_records(7, 6, 2, recv, stream=STREAM),
                 lambda: env.rollout_uniform(7, 7, 2, stream=STREAM), lambda: env.rollout_uniform(7, 8, 2, fused=False, stream=STREAM),
                 lambda: env.rollout_uniform_exchange(7, 9, 2, send, recv, stream=STREAM),
                 lambda: env.rollout_uniform_records(7, 10, 2, recv, stream=STREAM)):
        call()
    t = {"actions": env.actions, "players": env.players, "obs": env.obs, "reward": env._reward, "done": env._done,
         "masks": env.masks, "rows": rows, "other": other, "send0": send[0], "send1": send[1], "recv": recv}
    names = {v.data_ptr(): k for k, v in t.items()}
    out = []
    for name, args, _ in L.calls:
        if name.endswith("_invalidate"):
            continue
        flat = [a.value if hasattr(a, "value") else a for a in args]
        out.append((name, [names.get(a, "host" if isinstance(a, int) and a > 1 << 20 else a) for a in flat]))
    return out


def test_every_method_hands_its_entry_point_the_header_s_arguments(env):
    """Each bracketed method's call has as many arguments as _lib.SIGNATURES lists for its entry point, an int where
    the table has an integer and a pointer (or None) where it has a pointer, and the buffers in their places."""
    import ctypes

    calls = recorded_calls(env)
    assert [c[0] for c in calls] == [
        "mrts_reset_dev", "mrts_step_dev", "mrts_step_dev", "mrts_step_dev", "mrts_step_uniform_dev", "mrts_step_uniform_dev",
        "mrts_step_rows_dev", "mrts_step_fused_dev", "mrts_rollout_fused_dev", "mrts_rollout_fused_exchange_dev",
        "mrts_rollout_fused_records_dev", "mrts_rollout_uniform_dev", "mrts_rollout_uniform_dev",
        "mrts_rollout_uniform_exchange_dev", "mrts_rollout_uniform_records_dev"]
    for name, args in calls:
        argtypes = _lib.SIGNATURES[name][0]
        assert len(args) == len(argtypes), name
        for a, t in zip(args[1:], argtypes[1:]):
            if t in (ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64):
                assert isinstance(a, int), (name, a)
            else:
                assert a is None or isinstance(a, str), (name, a)  # a named buffer, host memory or a null pointer
    bufs = ["players", "obs", "reward", "done"]
    want = {
        0: ["handle"] + bufs + ["masks", 0, None],
        1: ["handle", "actions"] + bufs + ["masks", 0, None],
        2: ["handle", "other"] + bufs + [None, 0, None],
        3: ["handle", "actions"] + bufs + [None, 0, None],
        4: ["handle", "actions"] + bufs + [None, 0, 7, 1, None],
        5: ["handle", "actions"] + bufs + ["masks", 0, 7, 2, None],
        6: ["handle", "rows", 3] + bufs + ["masks", 0, None],
        7: ["handle", "actions"] + bufs + ["masks", 0, 7, 3, None],
        8: ["handle", "actions"] + bufs + ["masks", 0, 7, 4, 2, None],
        9: ["handle", "actions"] + bufs + ["masks", 0, 7, 5, 2, "send0", "send1", "recv", None],
        10: ["handle", "actions"] + bufs + ["masks", 0, 7, 6, 2, "recv", "host", None],
        11: ["handle", "actions"] + bufs + [7, 7, 2, 1, None],
        12: ["handle", "actions"] + bufs + [7, 8, 2, 0, None],
        13: ["handle", "actions"] + bufs + [7, 9, 2, "send0", "send1", "recv", None],
        14: ["handle", "actions"] + bufs + [7, 10, 2, "recv", "host", None],
    }
    for i, w in want.items():
        assert calls[i][1] == w, calls[i]


def test_random_policy_and_sample_actions_keep_their_own_rules(env):
    """random_policy tracks the tensor it wrote (any `out`) and invalidates for every other one; sample_actions
    leaves no tensor tracked; set_state_json and restore drop the tracked one."""
    L = env._h.L
    env.random_policy(7, 0, stream=STREAM)
    assert L.names() == ["mrts_policy_invalidate", "mrts_policy_dev"] and env._policy_out is env.actions
    env.random_policy(7, 1, stream=STREAM)
    assert L.names() == ["mrts_policy_dev"]
    env.actions.add_(1)
    env.random_policy(7, 2, stream=STREAM)
    assert L.names() == ["mrts_policy_invalidate", "mrts_policy_dev"]
    other = torch.zeros_like(env.actions)
    env.random_policy(7, 3, out=other, stream=STREAM)
    assert L.names() == ["mrts_policy_invalidate", "mrts_policy_dev"] and env._policy_out is other
    env.step_fused(7, 4, stream=STREAM)  # the tracked tensor is not env.actions: no invalidate
    assert L.names() == ["mrts_obs_invalidate", "mrts_step_fused_dev"] and env._policy_out is env.actions
    logits = torch.zeros((2, 16, 78))
    env.sample_actions(logits, 7, 5, stream=STREAM)
    assert L.names() == ["mrts_policy_head_sample_dev"] and (env._policy_out, env._policy_version) == (None, -1)
    env.actions.add_(1)
    env.step_fused(7, 6, stream=STREAM)  # nothing tracked: the library dropped its bases itself
    assert L.names() == ["mrts_step_fused_dev"]
    for drop in (lambda: env.set_state_json(0, "{}"), lambda: env.restore(b"x")):
        env.step_fused(7, 7, stream=STREAM)
        assert env._policy_out is env.actions
        env._h.set_state_json = env._h.restore = lambda *a: None
        env.synchronize = lambda: None
        drop()
        assert env._policy_out is None
        L.calls.clear()
