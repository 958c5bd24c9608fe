"""The shared comparators of tests/gpu_support.py and the dump reader of tests/dumps.py, on the CPU.

Almost every GPU test ends in assert_matches_oracle or assert_same_outputs: a comparator that compared nothing
would turn the suite green.  Here both run on stand-ins for a device env (CPU tensors filled from a real oracle
rollout of 4 slots on basesWorkers8x8): they pass on equal inputs, and for each output in turn one changed element
on one side makes them fail with a message that names that output.  Also: dumps.parse against a plain walk over
the raw words, and the one map writer against the text tests/test_gpu_issue_both.py used to write itself."""
import numpy as np
import pytest
import torch

from tests import dumps, oracle_py
from tests.defs import BASE, SEED, WORKER, write_map
from tests.gpu_support import Record, assert_matches_oracle, assert_same_outputs, same

MAP = "maps/8x8/basesWorkers8x8.xml"
S, STEPS = 4, 25


class Ref:
    """What the comparators read of an oracle, as plain arrays."""

    def __init__(self, obs, reward, done, masks, states, steps):
        self.obs, self.reward, self.done, self._masks, self._states, self._steps = obs, reward, done, masks, states, steps
        self.S = len(obs)

    def get_masks(self, player=0):
        assert player == 0
        return self._masks

    def dump(self, i):
        return self._states[i]

    def env_steps(self, i):
        return self._steps[i]

    def pick(self, slots):
        """A copy that holds these slots only, in this order."""
        return Ref(self.obs[slots].copy(), self.reward[slots].copy(), self.done[slots].copy(), self._masks[slots].copy(),
                   [self._states[s].copy() for s in slots], [self._steps[s] for s in slots])


class Env:
    """What the comparators read of a device env, on the CPU; `_h` is the handle's part of it."""

    def __init__(self, ref, rows):
        t = torch.from_numpy
        self.obs, self.reward, self.done = t(ref.obs.copy()), t(ref.reward.copy()), t(ref.done.copy())
        self.masks, self.actions = t(ref._masks.copy()), t(rows.copy())
        self.source = torch.arange(ref.S * 2, dtype=torch.int32).reshape(ref.S, 2)
        self.states = [d.copy() for d in ref._states]
        self.flags = np.zeros(ref.S, np.uint32)
        self.steps = np.asarray(ref._steps, np.int32).copy()
        self.S, self._h = ref.S, self

    def synchronize(self):
        pass

    def dump_state(self, s):
        return self.states[s]

    def error_flags(self):
        return self.flags

    def env_steps(self):
        return self.steps


@pytest.fixture(scope="module")
def rollout():
    """(Ref, next action rows [S][HW][7]) after STEPS masked-random steps: units have moved, assignments are under way."""
    o = oracle_py.OracleVecClient(S, 0, 2000, [MAP] * S, seed=3)
    o.reset()
    for step in range(STEPS):
        m = o.get_masks(0)
        o.step(np.stack([oracle_py.policy(m[s], SEED, s, step, 0) for s in range(S)]))
    m = o.get_masks(0)
    rows = np.stack([oracle_py.policy(m[s], SEED, s, STEPS, 0) for s in range(S)])
    ref = Ref(o.obs.copy(), o.reward.copy(), o.done.copy(), m, [o.dump(s) for s in range(S)], [o.env_steps(s) for s in range(S)])
    o.close()
    assert all(dumps.n_assign(d) > 0 for d in ref._states), "want assignments under way"
    return ref, rows


@pytest.fixture
def pair(rollout):
    """A fresh (env, ref, rows) for a test to damage."""
    ref, rows = rollout
    ref = ref.pick(list(range(S)))
    return Env(ref, rows), ref, rows


# one changed element of each compared output, in the env's slot s (a state's word 0 is its time)
DAMAGE = {
    "obs": lambda e, s: e.obs[s, 0, 0, 0].add_(1),
    "reward": lambda e, s: e.reward[s].add_(1),
    "done": lambda e, s: e.done[s].bitwise_xor_(1),
    "masks": lambda e, s: e.masks[s, 0, 0, 0].bitwise_xor_(1),
    "actions": lambda e, s: e.actions[s, 5, 0].add_(1),
    "source": lambda e, s: e.source[s, 1].add_(1),
    "state": lambda e, s: e.states[s].__setitem__(0, e.states[s][0] + 1),
    "env steps": lambda e, s: e.steps.__setitem__(s, e.steps[s] + 1),
    "error flags": lambda e, s: e.flags.__setitem__(s, 4),
}
# output -> how assert_matches_oracle's message names it (slot 2 is damaged)
ORACLE_OUTPUTS = {"obs": "obs", "reward": "reward", "done": "done", "masks": "masks", "actions": "next action rows",
                  "state": "state of slot 2", "env steps": "env steps of slot 2"}
# the same for assert_same_outputs
TWIN_OUTPUTS = {"obs": "obs", "masks": "masks", "actions": "actions", "source": "source", "reward": "reward", "done": "done",
                "error flags": "error flags differ", "env steps": "env steps", "state": "state of slot 2"}


def _full(env, ref, rows, **kw):
    assert_matches_oracle(env, ref, "t", next_rows=rows, env_steps=True, **kw)


def test_equal_inputs_pass(pair):
    env, ref, rows = pair
    _full(env, ref, rows)
    _full(env, ref, rows, states="even", xy_free=True)
    assert_matches_oracle(env, ref, "t", masks=None, rewards=None, states=None)
    assert_matches_oracle(env, ref, "t", next_rows=rows[:2])  # rows of the first slots only
    assert_same_outputs(env, Env(ref, rows), "t")


@pytest.mark.parametrize("name", list(ORACLE_OUTPUTS))
def test_oracle_comparator_fails_on_each_output(pair, name):
    env, ref, rows = pair
    DAMAGE[name](env, 2)
    with pytest.raises(AssertionError, match=f"t: {ORACLE_OUTPUTS[name]}"):
        _full(env, ref, rows)
    if name not in ("state", "env steps"):  # (those messages say "slot 2" by themselves)
        with pytest.raises(AssertionError, match=r"\(slot 2\)"):
            _full(env, ref, rows)


def test_oracle_comparator_options_switch_off_only_what_they_name(pair):
    env, ref, rows = pair
    for name, off in (("masks", dict(masks=None)), ("reward", dict(rewards=None)), ("done", dict(rewards=None)),
                      ("state", dict(states=None)), ("actions", {}), ("env steps", {})):
        e = Env(ref, rows)
        DAMAGE[name](e, 2)
        assert_matches_oracle(e, ref, "t", **off)
        with pytest.raises(AssertionError, match=ORACLE_OUTPUTS[name]):
            _full(e, ref, rows)
    e = Env(ref, rows)
    DAMAGE["state"](e, 1)  # an odd slot: "even" does not look at it, "all" does
    assert_matches_oracle(e, ref, "t", states="even")
    with pytest.raises(AssertionError, match="state of slot 1"):
        assert_matches_oracle(e, ref, "t", states="all")
    e = Env(ref, rows)
    DAMAGE["actions"](e, 3)  # rows of the first two slots: slot 3's are not looked at, slot 1's are
    assert_matches_oracle(e, ref, "t", next_rows=rows[:2])
    DAMAGE["actions"](e, 1)
    with pytest.raises(AssertionError, match="next action rows"):
        assert_matches_oracle(e, ref, "t", next_rows=rows[:2])


def test_first_reward_column(pair):
    env, ref, rows = pair
    wide = Ref(ref.obs, np.stack([ref.reward, ref.reward + 5], axis=1), np.stack([ref.done, 1 - ref.done], axis=1), ref._masks,
               ref._states, ref._steps)
    assert_matches_oracle(env, wide, "t", rewards="first")
    with pytest.raises(AssertionError, match="t: reward"):
        assert_matches_oracle(env, wide, "t")
    DAMAGE["done"](env, 0)
    with pytest.raises(AssertionError, match="t: done"):
        assert_matches_oracle(env, wide, "t", rewards="first")


@pytest.mark.parametrize("name", list(ORACLE_OUTPUTS))
def test_picked_slots(pair, name):
    """An oracle of two slots replays the env's slots 3 and 1: a difference in one of them fails and names the slot,
    the same difference in slot 0 or 2 is not looked at."""
    env, ref, rows = pair
    picks = [3, 1]
    sub, sub_rows = ref.pick(picks), rows[picks]
    check = lambda e: assert_matches_oracle(e, sub, "t", slots=picks, next_rows=sub_rows, env_steps=True)  # noqa: E731
    check(env)
    for outside in (0, 2):
        e = Env(ref, rows)
        DAMAGE[name](e, outside)
        check(e)
    for inside in picks:
        e = Env(ref, rows)
        DAMAGE[name](e, inside)
        with pytest.raises(AssertionError, match=f"t: {ORACLE_OUTPUTS[name].split(' of slot')[0]}.*slot {inside}"):
            check(e)
    with pytest.raises(AssertionError, match="3 slots picked for an oracle of 2"):
        assert_matches_oracle(env, sub, "t", slots=[3, 1, 0])


@pytest.mark.parametrize("name", list(TWIN_OUTPUTS))
def test_twin_comparator_fails_on_each_output(pair, name):
    env, ref, rows = pair
    twin = Env(ref, rows)
    DAMAGE[name](twin, 2)
    with pytest.raises(AssertionError, match=f"t: {TWIN_OUTPUTS[name]}"):
        assert_same_outputs(env, twin, "t")


@pytest.mark.parametrize("name", list(TWIN_OUTPUTS))
def test_a_record_holds_an_env_to_an_earlier_moment(pair, name):
    """Record copies: the env it was taken from equals it until one of its outputs changes, whichever it is."""
    env, ref, rows = pair
    rec = Record(env)
    assert_same_outputs(env, rec, "t")
    assert_same_outputs(Env(ref, rows), rec, "t")
    DAMAGE[name](env, 2)
    with pytest.raises(AssertionError, match=f"t: {TWIN_OUTPUTS[name]}"):
        assert_same_outputs(env, rec, "t")


def test_twin_comparator_wants_the_error_flags_unset(pair):
    env, ref, rows = pair
    twin = Env(ref, rows)
    DAMAGE["error flags"](env, 1)
    DAMAGE["error flags"](twin, 1)
    with pytest.raises(AssertionError, match="t: error flags set"):
        assert_same_outputs(env, twin, "t")


def test_same_reports_shape_dtype_and_the_first_difference():
    a = torch.zeros((2, 3), dtype=torch.int32)
    same(a, np.zeros((2, 3), np.int32), "x", "t")
    with pytest.raises(AssertionError, match=r"t: x int32\(2, 3\) vs int64\(2, 3\)"):
        same(a, np.zeros((2, 3), np.int64), "x", "t")
    with pytest.raises(AssertionError, match=r"t: x int32\(2, 3\) vs int32\(3, 2\)"):
        same(a, np.zeros((3, 2), np.int32), "x", "t")
    b = np.zeros((2, 3), np.int32)
    b[1, 0], b[1, 2] = 7, 9
    with pytest.raises(AssertionError, match=r"t: x differs at 2 places, first \[1, 0\] \(slot 5\): gpu 0 ref 7"):
        same(a, b, "x", "t", slots=[4, 5])


def _with_assignment_type(d, k, t, x):
    """dump d with assignment k's action type and x replaced"""
    s = dumps.parse(d)
    s.assign[k, 1], s.assign[k, 3] = t, x
    return dumps.build(*s)


def test_xy_free_ignores_x_y_of_all_but_attacks(pair):
    env, ref, rows = pair
    d = ref._states[0]
    kind = int(dumps.parse(d).assign[0, 1])
    assert kind != dumps.ATTACK
    ref._states[0], env.states[0] = _with_assignment_type(d, 0, kind, -1), _with_assignment_type(d, 0, kind, 0)
    assert_matches_oracle(env, ref, "t", xy_free=True)
    with pytest.raises(AssertionError, match="state of slot 0"):
        assert_matches_oracle(env, ref, "t")
    ref._states[0], env.states[0] = _with_assignment_type(d, 0, dumps.ATTACK, 3), _with_assignment_type(d, 0, dumps.ATTACK, 4)
    with pytest.raises(AssertionError, match="state of slot 0"):
        assert_matches_oracle(env, ref, "t", xy_free=True)


def test_parse_field_by_field(rollout):
    """dumps.parse and the accessors against a plain walk over the words of a real mid-game dump."""
    d = rollout[0]._states[0]
    s = dumps.parse(d)
    w = iter(d.tolist())
    assert s.time == next(w) == STEPS and next(w) == 2
    assert s.res == (next(w), next(w))
    nu = next(w)
    assert nu == dumps.n_units(d) == len(s.units) > 2 and s.units.shape == (nu, 6)
    for u in s.units.tolist():
        assert u == [next(w) for _ in range(6)]
    na = next(w)
    assert na == dumps.n_assign(d) == len(s.assign) > 0 and s.assign.shape == (na, 7)
    for k, a in enumerate(s.assign.tolist()):
        assert a == [next(w) for _ in range(7)]
        row, place = dumps.assignment_of(d, a[0])
        assert row.tolist() == a and place == k
    assert next(w, None) is None, "words left over"
    assert np.array_equal(dumps.live_units(d), s.units)
    idle = sorted(set(range(nu)) - set(s.assign[:, 0].tolist()))
    assert idle and dumps.assignment_of(d, idle[0]) is None
    with pytest.raises(AssertionError, match="words"):
        dumps.parse(d[:-1])
    assert np.array_equal(dumps.build(*s), d)
    free = dumps.parse(dumps.xy_free(d))
    assert np.array_equal(free.units, s.units) and np.array_equal(free.assign[:, :3], s.assign[:, :3])
    assert not free.assign[free.assign[:, 1] != dumps.ATTACK][:, 3:5].any() and np.array_equal(d, rollout[0]._states[0])


# tests/test_gpu_issue_both.py's scenario map: its unit list, and the text that file wrote itself before it
# called defs.write_map (unit IDs from 10, no line break after the last attribute)
ISSUE_BOTH_UNITS = [(BASE, 0, 1, 1), (BASE, 0, 1, 4), (WORKER, 0, 3, 2), (WORKER, 0, 3, 4), (WORKER, 0, 2, 6), (BASE, 1, 6, 6),
                    (BASE, 1, 7, 3), (WORKER, 1, 5, 2), (WORKER, 1, 5, 4), (WORKER, 1, 4, 6)]


def _former_issue_both_map(path, size):
    units = "".join(f'    <rts.units.Unit type="{"Base" if t == BASE else "Worker"}" ID="{10 + i}" player="{p}" x="{x}" y="{y}" '
                    f'resources="0" hitpoints="{10 if t == BASE else 1}" >\n    </rts.units.Unit>\n'
                    for i, (t, p, x, y) in enumerate(ISSUE_BOTH_UNITS))
    path.write_text(f'<rts.PhysicalGameState width="{size}" height="{size}">\n  <terrain>{"0" * (size * size)}</terrain>\n'
                    '  <players>\n    <rts.Player ID="0" resources="1">\n    </rts.Player>\n'
                    '    <rts.Player ID="1" resources="5">\n    </rts.Player>\n  </players>\n  <units>\n'
                    f'{units}  </units>\n</rts.PhysicalGameState>\n')
    return str(path)


@pytest.mark.parametrize("size", [8, 16, 10])
def test_the_one_map_writer_gives_the_former_issue_both_map(tmp_path, size):
    """The two writers differ in the XML unit IDs (100 + i against 10 + i) and in whitespace only: the oracle's reset
    state, observation and masks of the two files are equal, on every size test_directed_steps runs."""
    new = write_map(tmp_path / "new.xml", size, size, ISSUE_BOTH_UNITS, res=(1, 5))
    old = _former_issue_both_map(tmp_path / "old.xml", size)
    assert open(new).read() != open(old).read()
    o = oracle_py.OracleVecClient(4, 0, 2000, [new, new, old, old], seed=11)
    obs, _, _ = o.reset()
    m = o.get_masks(0)
    assert dumps.parse(o.dump(0)).res == (1, 5) and dumps.n_units(o.dump(0)) == len(ISSUE_BOTH_UNITS)
    assert np.array_equal(o.dump(0), o.dump(2)), f"reset state\n{o.dump(0).tolist()}\n{o.dump(2).tolist()}"
    assert np.array_equal(obs[:2], obs[2:]) and np.array_equal(m[:2], m[2:]) and m[:2].any()
    o.close()
