"""selfPlayFast's merged issue pass (MRTS_ISSUE_BOTH) against the CPU oracle, bit-exact.

Both players' accepted rows are issued in one pass when no candidate row of either interacts with a
reservation or with another row; otherwise the per-player passes run as before.  The tests drive steps on
both sides of that test — clean steps, cross-player and same-player target clashes, a reservation in flight,
PRODUCE sums over the resources, a bad produce type — on the 8x8, the 16x16 and the generic kernel, and the
fused multi-step path of the headline workload, and compare observations, rewards, dones, masks and the full
state dump (whose assignment order carries the sequence numbers) after every step.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import dumps, oracle_py
from tests.defs import BASE, DOWN, DX, DY, LEFT, RIGHT, SEED, UP, WORKER, write_map
from tests.defs import MOVE as T_MOVE, PRODUCE as T_PRODUCE
from tests.gpu_checks import FUSED_MAP, flag_rollout
from tests.gpu_support import assert_matches_oracle, assert_same_outputs, torch_gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_PRODUCE_TYPE = 1 << 2


# The scenarios' map (the reference's XML layout, PhysicalGameState.java:700-726), within the top-left 8x8
# cells of any size: two Bases and three Workers per player, player 0 with 1 resource (one Worker's cost),
# player 1 with 5.
#   y\x 0  1  2  3  4  5  6  7
#   1      A0
#   2            P     S
#   3                        B1
#   4      A1    Q     T
#   6         R     U     B0
UNITS = {"A0": (BASE, 0, 1, 1), "A1": (BASE, 0, 1, 4), "P": (WORKER, 0, 3, 2), "Q": (WORKER, 0, 3, 4),
         "R": (WORKER, 0, 2, 6), "B0": (BASE, 1, 6, 6), "B1": (BASE, 1, 7, 3), "S": (WORKER, 1, 5, 2),
         "T": (WORKER, 1, 5, 4), "U": (WORKER, 1, 4, 6)}


def _write_map(tmp_path, size):
    return write_map(tmp_path / f"issue_both{size}x{size}.xml", size, size, list(UNITS.values()), res=(1, 5))


def _row(kind, d=0, ut=0):
    r = [kind, 0, 0, 0, 0, 0, 0]
    if kind == T_MOVE:
        r[1] = d
    elif kind == T_PRODUCE:
        r[4], r[5] = d, ut
    return r


MOVE = lambda d: _row(T_MOVE, d)  # noqa: E731
PROD = lambda d, ut=WORKER: _row(T_PRODUCE, d, ut)  # noqa: E731
NONE = _row(0)

# scenario -> the scripted steps: {unit: row}; units left out get a NONE row
SCENARIOS = {
    # every target distinct and free, one PRODUCE per player within its resources, R / U / A1 / B1 idle with NONE
    # rows: the merged pass, sequence layout [accepted 0][fills 0][accepted 1][fills 1]
    "clean": [{"P": MOVE(RIGHT), "Q": MOVE(LEFT), "S": MOVE(DOWN), "T": MOVE(RIGHT), "A0": PROD(RIGHT), "B0": PROD(UP)}],
    # P and S both into (4,2): player 0's is accepted, player 1's is dropped by its chain and filled with NONE(1)
    "cross_target": [{"P": MOVE(RIGHT), "S": MOVE(LEFT), "Q": MOVE(LEFT), "T": MOVE(RIGHT)}],
    # P and Q both into (3,3); player 1 clean
    "dup_target_p0": [{"P": MOVE(DOWN), "Q": MOVE(UP), "S": MOVE(RIGHT), "B0": PROD(UP)}],
    # S and T both into (5,3); player 0 clean
    "dup_target_p1": [{"S": MOVE(DOWN), "T": MOVE(UP), "P": MOVE(LEFT), "A0": PROD(RIGHT)}],
    # step 1: P starts a MOVE into (4,2) (10 cycles); step 2: S moves into the reserved cell
    "reservation": [{"P": MOVE(RIGHT)}, {"S": MOVE(LEFT), "Q": MOVE(LEFT), "T": MOVE(RIGHT)}],
    # player 0 holds 1 resource: A0's Worker is accepted, A1's is rejected (1 + 1 > 1); player 1's one PRODUCE fits
    "produce_sums": [{"A0": PROD(RIGHT), "A1": PROD(RIGHT), "B0": PROD(UP), "P": MOVE(RIGHT), "S": MOVE(DOWN)}],
    # A0's row names a produce type outside the table: the unit goes to the fills, E_PRODUCE_TYPE is flagged
    "bad_type_p0": [{"A0": PROD(RIGHT, 7), "P": MOVE(RIGHT), "S": MOVE(DOWN), "B0": PROD(UP)}],
    "bad_type_p1": [{"B0": PROD(UP, 9), "P": MOVE(RIGHT), "S": MOVE(DOWN), "A0": PROD(RIGHT)}],
}


def _scripted_actions(S, size, step_rows):
    acts = np.zeros((S, size * size, 7), np.int32)
    for name, row in step_rows.items():
        _, p, x, y = UNITS[name]
        acts[p::2, y * size + x] = row  # slot 2g = game g's player 0, slot 2g + 1 = its player 1
    return acts


def _assert_same(env, ref, tag):
    assert_matches_oracle(env, ref, tag, states="even")


def _assignment_of(ref, name):
    """(type, parameter, insertion index) of the unit's assignment in the oracle's game 0, or None"""
    d = ref.dump(0)
    _, p, x, y = UNITS[name]
    idx = [i for i, u in enumerate(dumps.live_units(d)) if (u[1], u[2], u[3]) == (p, x, y)]
    assert len(idx) == 1, f"{name} is not where the map put it"
    held = dumps.assignment_of(d, idx[0])
    return held and (int(held[0][1]), int(held[0][2]), held[1])


def _oracle_scripted_step(ref, acts, step_rows, size):
    bad = [n for n, r in step_rows.items() if r[0] == T_PRODUCE and r[5] >= 7]
    if not bad:
        ref.step(acts)
        return
    # Java's fromVectorAction throws on a produce type outside the table (UnitTypeTable.getUnitType), and so
    # does the oracle; the kernels flag E_PRODUCE_TYPE and treat the unit as one without a row (fillWithNones
    # gives it NONE(1)): the oracle takes the same rows in cell order without that cell's
    cellb = UNITS[bad[0]][3] * size + UNITS[bad[0]][2]
    cells = [c for c in range(size * size) if c != cellb]
    S = acts.shape[0]
    rows = np.concatenate([np.broadcast_to(np.asarray(cells, np.int32)[None, :, None], (S, len(cells), 1)),
                           acts[:, cells]], axis=2)
    ref.step_rows(rows)


def _check_intent(ref, scenario):
    """what the scenario is for, read from the oracle's state after its scripted steps"""
    # (the step's cycle has run: NONE assignments, the fills' NONE(1) included, are over and gone; a row that was
    # dropped or filled shows as a unit without an assignment, the insertion order on those that remain)
    if scenario == "clean":
        # player 0's rows by cell, then player 1's by cell
        order = [_assignment_of(ref, n)[2] for n in ("A0", "P", "Q", "S", "T", "B0")]
        assert order == list(range(6)), order
        assert _assignment_of(ref, "A0")[0] == T_PRODUCE and _assignment_of(ref, "B0")[0] == T_PRODUCE
        assert all(_assignment_of(ref, n) is None for n in ("R", "U", "A1", "B1"))
    elif scenario == "cross_target":
        assert _assignment_of(ref, "P")[:2] == (T_MOVE, RIGHT) and _assignment_of(ref, "S") is None
        assert _assignment_of(ref, "Q")[0] == T_MOVE and _assignment_of(ref, "T")[0] == T_MOVE
    elif scenario == "dup_target_p0":
        assert _assignment_of(ref, "P")[:2] == (T_MOVE, DOWN) and _assignment_of(ref, "Q") is None
        assert _assignment_of(ref, "S")[0] == T_MOVE and _assignment_of(ref, "B0")[0] == T_PRODUCE
    elif scenario == "dup_target_p1":
        assert _assignment_of(ref, "S")[:2] == (T_MOVE, DOWN) and _assignment_of(ref, "T") is None
        assert _assignment_of(ref, "P")[0] == T_MOVE and _assignment_of(ref, "A0")[0] == T_PRODUCE
    elif scenario == "reservation":
        assert _assignment_of(ref, "P")[:2] == (T_MOVE, RIGHT)  # still in flight
        assert _assignment_of(ref, "S") is None and _assignment_of(ref, "T")[:2] == (T_MOVE, RIGHT)
    elif scenario == "produce_sums":
        assert _assignment_of(ref, "A0")[0] == T_PRODUCE and _assignment_of(ref, "A1") is None
        assert _assignment_of(ref, "B0")[0] == T_PRODUCE
    else:
        name, other = ("A0", "B0") if scenario == "bad_type_p0" else ("B0", "A0")
        assert _assignment_of(ref, name) is None and _assignment_of(ref, other)[0] == T_PRODUCE
        assert _assignment_of(ref, "P")[0] == T_MOVE and _assignment_of(ref, "S")[0] == T_MOVE


@pytest.mark.parametrize("size", [8, 16, 10])
@pytest.mark.parametrize("scenario", list(SCENARIOS))
def test_directed_steps(tmp_path, scenario, size):
    """One scripted step (two for the reservation in flight) through env.step() — rows from the action tensor,
    issueSafe's legality test on — then 20 masked-random steps, on 4 games; every step against the oracle.
    The oracle's own state asserts what the scenario is for (who was accepted, who was filled), so the
    comparison cannot pass on a scenario that does not happen."""
    torch = torch_gpu()
    from microrts_amd import DeviceVecEnv

    S = 8
    mp = _write_map(tmp_path, size)
    env = DeviceVecEnv(S, 0, 2000, [mp] * S, seed=11)
    ref = oracle_py.OracleVecClient(S, 0, 2000, [mp] * S, seed=11)
    env.reset()
    ref.reset()
    _assert_same(env, ref, "reset")
    bad = scenario.startswith("bad_type")
    for k, step_rows in enumerate(SCENARIOS[scenario]):
        acts = _scripted_actions(S, size, step_rows)
        env.actions.copy_(torch.as_tensor(acts))
        env.step()
        _oracle_scripted_step(ref, acts, step_rows, size)
        _assert_same(env, ref, f"{scenario} scripted step {k + 1}")
    _check_intent(ref, scenario)
    for step in range(20):
        env.random_policy(SEED, step)
        env.synchronize()
        acts = env.actions.cpu().numpy()
        env.step()
        ref.step(acts)
        _assert_same(env, ref, f"{scenario} random step {step + 1}")
    flags = env.error_flags()
    assert (flags == (E_PRODUCE_TYPE if bad else 0)).all(), flags
    env.close()
    ref.close()


def _clash(dump, rows0, rows1, W):
    """Does this game-step keep the merged pass from being taken on positions: two candidate rows (idle units'
    MOVE / PRODUCE rows, either player) with one target cell, or one targeting a cell an assignment in flight
    has reserved?  From the oracle's state before the step and the step's rows."""
    _, _, units, asg = dumps.parse(dump)
    busy = {int(a[0]) for a in asg}
    taken = set()
    for a in asg:
        if a[1] in (T_MOVE, T_PRODUCE):
            u = units[a[0]]
            taken.add((u[2] + DX[a[2]], u[3] + DY[a[2]]))
    for i, u in enumerate(units):
        if i in busy or u[1] < 0:
            continue
        r = (rows0 if u[1] == 0 else rows1)[u[3] * W + u[2]]
        if r[0] == T_MOVE or r[0] == T_PRODUCE:
            d = r[1] if r[0] == T_MOVE else r[4]
            tgt = (u[2] + DX[d], u[3] + DY[d])
            if tgt in taken:
                return True
            taken.add(tgt)
    return False


FUSED_LAUNCHES = (1, 3, 40, 57, 2, 97, 64, 136)  # 400 steps
FUSED_SEED = 5


def test_fused_multi_step_rollout():
    """The headline's own path — forwarded rows, legality skipped, several steps per launch: 32 self-play games
    on basesWorkers16x16 for 400 steps in launches of uneven length, against a twin stepped one launch per
    step and against the oracle at every launch boundary (outputs, next rows, every game's state).  The
    oracle's side asserts that the rollout holds at least 20 game-steps with a target clash among the candidate
    rows or with a reservation in flight, so both the merged pass and the per-player passes ran."""
    torch_gpu()
    from microrts_amd import DeviceVecEnv

    S = 64
    mk = lambda: DeviceVecEnv(S, 0, 2000, [FUSED_MAP] * S, seed=FUSED_SEED)  # noqa: E731
    A, B = mk(), mk()
    A.set_multi_step(False)
    assert B.fused_multi_step
    ref = oracle_py.OracleVecClient(S, 0, 2000, [FUSED_MAP] * S, seed=FUSED_SEED)
    ref.reset()
    for e in (A, B):
        e.reset()
        e.random_policy(SEED, 0)
    W = ref.W
    k, clashes, clean = 0, 0, 0
    for n in FUSED_LAUNCHES:
        A.rollout_fused(SEED, k + 1, n)
        B.rollout_fused(SEED, k + 1, n)
        for t in range(k, k + n):
            m = ref.get_masks(0)
            acts = np.stack([oracle_py.policy(m[s], SEED, s, t, 0) for s in range(S)])
            if clashes < 20 or clean < 20:
                for g in range(S // 2):
                    c = _clash(ref.dump(2 * g), acts[2 * g], acts[2 * g + 1], W)
                    clashes += c
                    clean += not c
            ref.step(acts)
        k += n
        tag = f"after the launch to step {k}"
        assert_same_outputs(A, B, f"{tag}: one launch per step vs multi-step")
        m = ref.get_masks(0)
        nxt = np.stack([oracle_py.policy(m[s], SEED, s, k, 0) for s in range(S)])
        assert_matches_oracle(B, ref, tag, next_rows=nxt, states="even")
        assert_matches_oracle(A, ref, f"{tag} (one launch per step)", masks=None, rewards=None, states="even")
    assert clashes >= 20 and clean >= 20, (clashes, clean)
    assert not A.error_flags().any() and not B.error_flags().any()
    A.close()
    B.close()
    ref.close()


def test_flag_off_equals_flag_on(tmp_path):
    """The library built with -DMRTS_ISSUE_BOTH=0 (`make x1 XFLAGS1=-DMRTS_ISSUE_BOTH=0`, loaded by a child
    process through MRTS_LIB_PATH) leaves the same observations, masks, rows, rewards, dones and state dumps
    as the default build over a 200-step fused rollout."""
    from microrts_amd import _lib

    x1 = os.path.join(ROOT, "microrts_amd", "libmrts_x1.so")
    if not os.path.exists(x1):
        pytest.skip("microrts_amd/libmrts_x1.so is not built (make -C microrts_amd/csrc x1 XFLAGS1=-DMRTS_ISSUE_BOTH=0)")
    if os.path.abspath(_lib.LIB_PATH) == x1:
        pytest.skip("this session's own library is the variant")
    off, on = str(tmp_path / "off.npz"), str(tmp_path / "on.npz")
    env = dict(os.environ, MRTS_LIB_PATH=x1)
    r = subprocess.run([sys.executable, "-c", f"from tests.gpu_checks import flag_rollout; flag_rollout({off!r})"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    flag_rollout(on)
    a, b = np.load(off), np.load(on)
    assert sorted(a.files) == sorted(b.files)
    for name in a.files:
        assert np.array_equal(a[name], b[name]), name
    assert not b["flags"].any()
