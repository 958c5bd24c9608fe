"""tests/error_cases.py on the oracle alone: every scenario happens, at the step it names, and its NONE twin runs
clean; every state is one the product's own converter takes (mrts_internal_state_probe).  The unit counts asserted
here are what say which of the kernels' three cycle() paths a scenario reaches on the GPU (tests/test_gpu_error_flags.py):
one unit per lane (at most 64 units), the LDS ready list (more than 64 units, at most 64 of them owned, so at most 64
ready; the 64 producers of the capacity case, every other owned unit busy) or the repeated minimum search (more than 64
ready: its 66 producers).  No GPU call."""
import json

import numpy as np
import pytest

from tests import dumps, oracle_py
from tests import error_cases as EC
from tests import state_cases as SC
from tests.defs import NONE, WORKER

STEPS = 25


def _probe_ok(size, text, max_units=0):
    n, out, err = SC.state_probe("mrts_internal_state_probe", size, max_units, text)
    assert n > 0, err
    assert len(json.loads(out.tobytes()[:n].decode())["pgs"]["units"]) == len(json.loads(text)["pgs"]["units"])


def _path(c, dump):
    units, owned = EC.counts(dump)
    if c[1] is None:
        assert units + 1 <= 64, "one unit per lane, the birth included"
    else:
        assert owned <= 64 < units, f"the LDS ready list: {units} units, {owned} owned"


@pytest.mark.parametrize("c", EC.NEG_CASES, ids=EC.case_id)
def test_neg_resources_happens(c):
    size, seed = c
    po = size == (32, 32)
    faulty, twin, fires_at = EC.neg_resources(size, crowd_seed=seed)
    for t in (faulty, twin):
        _probe_ok(size, t, EC.PO_MAX_UNITS if po else 0)
    ref = EC.oracle(size, EC.games(size, faulty), partial_obs=po)
    bad = [s for g in EC.FAULTY for s in (2 * g, 2 * g + 1)]
    for step in range(STEPS):
        if step == fires_at - 1:
            for g in EC.FAULTY:
                _path(c, ref.dump(2 * g))
                a, _ = dumps.assignment_of(ref.dump(2 * g), _base(ref.dump(2 * g)))
                assert a[1] == 4 and a[5] == WORKER, "the production is still under way"
        ref.step(EC.masked_rows(ref, step))
        e = EC.errors(ref)
        want = np.zeros(ref.S, int)
        want[bad] = step + 1 >= fires_at
        assert np.array_equal(e, want), f"step {step}: Java's prints per slot {e.tolist()}"
        if step == fires_at - 1:
            for g in EC.FAULTY:
                d = ref.dump(2 * g)
                assert dumps.assignment_of(d, _base(d)) is None and dumps.parse(d).res[0] == 0, "skipped, nothing paid"
    assert not ref.done.any()
    ref.close()


def _base(dump):
    u = dumps.live_units(dump)
    return int(np.nonzero((u[:, 0] == 1) & (u[:, 1] == 0))[0][0])


def test_neg_resources_against_a_bot():
    faulty, _, fires_at = EC.neg_resources((10, 10))
    ref = EC.oracle((10, 10), EC.games((10, 10), faulty), bots=True)
    for step in range(STEPS):
        ref.step(EC.masked_rows(ref, step))
        want = np.zeros(ref.S, int)
        want[list(EC.FAULTY)] = step + 1 >= fires_at
        assert np.array_equal(EC.errors(ref), want), step
    ref.close()


@pytest.mark.parametrize("c", EC.ADDUNIT_CASES, ids=EC.case_id)
def test_addunit_happens(c):
    size, seed = c
    faulty, twin, fires_at = EC.addunit(size, crowd_seed=seed)
    assert fires_at == 1
    for t in (faulty, twin):
        _probe_ok(size, t)
    ref = EC.oracle(size, EC.games(size, faulty))
    for g in EC.FAULTY:
        _path(c, ref.dump(2 * g))
        units, owned = EC.counts(ref.dump(2 * g))
        assert owned <= 64, "zero rows give every idle owned unit a NONE that is ready at once: still at most 64 ready"
    with pytest.raises(RuntimeError, match="added two units in position"):
        ref.step(EC.zero_rows(ref))
    ref.close()
    ref = EC.oracle(size, EC.games(size, twin))
    before = [dumps.parse(ref.dump(2 * g)) for g in EC.FAULTY]
    ref.step(EC.zero_rows(ref))
    for g, b in zip(EC.FAULTY, before):
        d = ref.dump(2 * g)
        st = dumps.parse(d)
        assert dumps.assignment_of(d, _base(d)) is None and st.res == b.res and np.array_equal(st.units, b.units), \
            "the NONE is over: nothing produced, nothing paid"
    for step in range(20):
        ref.step(EC.masked_rows(ref, step))
    assert not EC.errors(ref).any()
    ref.close()


@pytest.mark.parametrize("size", EC.COLLISION_SIZES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_collision_happens(size):
    faulty, twin, fires_at = EC.collision(size)
    assert fires_at == 1
    for t in (faulty, twin):
        _probe_ok(size, t)
    ref = EC.oracle(size, EC.games(size, faulty))
    ref.step(EC.zero_rows(ref))
    assert not EC.errors(ref).any(), "Java moves the unit without a word"
    for g in range(EC.GAMES):
        u = dumps.live_units(ref.dump(2 * g))
        cells = [tuple(c) for c in u[:, 2:4].tolist()]
        assert (len(set(cells)) < len(cells)) == (g in EC.FAULTY), f"game {g}: two units on one cell"
    ref.close()
    ref = EC.oracle(size, EC.games(size, twin))
    ref.step(EC.zero_rows(ref))
    for step in range(10):
        ref.step(EC.masked_rows(ref, step))
    assert not EC.errors(ref).any()
    ref.close()


@pytest.mark.parametrize("producers", [64, 66])
def test_capacity_happens(producers):
    """All `producers` births land on the oracle (it has no capacity): that many assignments were ready in one cycle.
    The twin of the 66 lands the first 64, in list order, and pays for 64."""
    faulty, twin, fires_at = EC.capacity(producers)
    M, size = EC.CAPACITY_UNITS, EC.CAPACITY_SIZE
    assert fires_at == 1
    for t in (faulty, twin):
        _probe_ok(size, t, M)
    n, _, err = SC.state_probe("mrts_internal_state_probe", size, M - 1, faulty)
    assert n == -28 and "max_units" in err, "exactly max_units units"
    states = EC.games(size, faulty, max_units=M)
    assert max(dumps.n_units(np.asarray(SC.state_probe("mrts_internal_dump_probe", size, M, s)[1])) for s in states) == M
    for text, births in ((faulty, producers), (twin, 64)):
        ref = EC.oracle(size, EC.games(size, text, max_units=M))
        st = dumps.parse(ref.dump(2 * EC.FAULTY[0]))
        assert EC.counts(ref.dump(2 * EC.FAULTY[0])) == (M, producers + 2) and M > 64
        kinds = [(int(a[1]), int(a[2])) for a in st.assign]
        assert kinds.count((NONE, EC.BUSY)) == 2 and len(kinds) == producers + 2, "no owned unit is idle: what is ready in the " \
            "firing cycle is what completes then, the producers' assignments (64: the LDS ready list; 66: past it)"
        ref.step(EC.zero_rows(ref))
        assert not EC.errors(ref).any() and not ref.done.any()
        for g in EC.FAULTY:
            st = dumps.parse(ref.dump(2 * g))
            assert len(st.units) == M + births and st.res == (100 - births, 5)
            born = st.units[M:]
            assert (born[:, 0] == WORKER).all() and (born[:, 1] == 0).all()
            assert born[:, 2:4].tolist() == [[x + 1, y] for y in range(9) for x in range(0, 16, 2)][:births], "in list order"
            assert not [a for a in st.assign if a[0] < producers], "every producer's assignment is over"
        ref.close()
    assert M + 64 == M + max(64, M // 4), "64 births fill the handle's unit slots exactly"


def test_older_conflict_trace():
    """The hand-written trace: the strict replay refuses it at the entry whose only action issue() turns down, the
    lenient one goes on, counts Java's print there and leaves Light 33 a NONE of parameter -1."""
    import os

    mp = os.path.join(SC.ROOT, EC.OLDER_MAP)
    with pytest.raises(RuntimeError, match="containsRealActions != issuedActions at time 10"):
        oracle_py.trace_dumps(mp, EC.OLDER_CONFLICT_TRACE)
    ds, issued, errs = oracle_py.trace_dumps(mp, EC.OLDER_CONFLICT_TRACE, lenient=True)
    assert issued.tolist() == [1, 1, 0, 0, 0] and errs.tolist() == [0, 0, 1, 1, 1]
    assert [dumps.parse(d).time for d in ds] == [0, 8, 10, 10, 20]
    assert dumps.assignment_of(ds[EC.OLDER_ENTRY], 1) is None
    a, _ = dumps.assignment_of(ds[EC.OLDER_ENTRY + 1], 1)
    assert a[1] == NONE and a[2] == -1 and a[6] == 10
    older, _ = dumps.assignment_of(ds[EC.OLDER_ENTRY], 0)
    assert older[1] == 1 and older[2] == 2 and older[6] == 8, "Light 32's MOVE DOWN of time 8 is under way"
    assert dumps.assignment_of(ds[4], 1) is None
    assert dumps.live_units(ds[4])[:, 2:4].tolist() == [[1, 1], [0, 1], [3, 2], [3, 3]]
