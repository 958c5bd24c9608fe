"""Packed policy rows on the GPU (mrts_policy_head_pack_dev / _unpack_dev / _score_packed_dev / _grad_packed_dev,
DeviceVecEnv.pack_step / unpack, evaluate_actions_packed) against the numpy packer of tests/policy_head_packed_ref.py
and, for the score and the gradient, against the dense kernels: the same bytes, compared as int32.

Shapes: 8x8 (one 64-cell chunk), NoWhereToRun9x8 (72 cells: a short last chunk), basesWorkers16x16 (four chunks).
Tables: the built-in one (K = 79) on these; tests/table_cases.py's r3, r5, t5r3 and t8r5 (K = 39, 55, 37, 56) on 4x4
and 9x8, as cases "4x4-r3" ...  nt and K come from the handle.
Rows: a 16-slot rollout of 50 steps driven by sample_actions (its last T steps with a candidate kept dense and
packed), and the synthetic rows of policy_head_packed_ref.synthetic_rows (no candidate; 1, 4, 5, 64 candidates in a chunk; both sides of a chunk
boundary; every cell; an empty field; components off the mask, -1 and 2^30; junk at non-candidate cells)."""
import ctypes
import math

import numpy as np
import pytest

from tests import policy_head_packed_ref as PR, table_cases as TC
from tests.gpu_support import ptr, torch_gpu

pytestmark = pytest.mark.gpu

MAPS = {"8x8": "maps/8x8/basesWorkers8x8.xml", "9x8": "maps/NoWhereToRun9x8.xml", "16x16": "maps/16x16/basesWorkers16x16.xml"}
TABLE_MAPS = {"4x4": "maps/4x4/basesWorkers4x4.xml", "9x8": MAPS["9x8"]}
CASES = list(MAPS) + [f"{shape}-{t}" for t in TC.IDS for shape in TABLE_MAPS]
S, T, STEPS = 16, 4, 50
HSEED = 0x0123456789ABCDEF


def _bits(t):
    return t.contiguous().view(torch_gpu().int32)


def _u32(shape, value, device):
    """a uint32 tensor filled with one word"""
    torch = torch_gpu()
    return torch.full(shape, value - (1 << 32) if value >> 31 else value, dtype=torch.int32, device=device).view(torch.uint32)


def _np32(t):
    return t.cpu().view(torch_gpu().int32).numpy().view(np.uint32)


class Case:
    """one shape and table ("9x8", "9x8-r5"): a rollout under sample_actions whose last T steps are kept dense and
    packed, and the synthetic rows"""

    def __init__(self, name):
        torch = torch_gpu()
        from microrts_amd import DeviceVecEnv, UnitTypeTable

        shape, _, table = name.partition("-")
        utt = UnitTypeTable.fromJSON(TC.utt_json(table)) if table else UnitTypeTable()
        self.env = env = DeviceVecEnv(S, 0, 2000, [(TABLE_MAPS if table else MAPS)[shape]] * S, seed=3, utt=utt)
        _, H, W, _, K = env.dims
        # the handle's own type count: its one-hot observation has 5 + 5 + 3 + (nt + 1) + 6 + 2 features
        self.HW, self.K, self.nt = H * W, K, env._h.L.mrts_onehot_features(env._h.h) - 22
        assert (self.nt, K) == ((TC.TABLES[table].nt, TC.TABLES[table].K) if table else (7, 79))
        assert not (table and env.multi_step_capable), "only the K = 79 instances run several steps per launch"
        dev = env.device
        g = torch.Generator().manual_seed(H * W)
        self.buf = env.packed_buffer(T)
        self.cap = (self.buf.shape[-1] - 1) // 5
        # the last T steps that had a candidate (on the small maps every unit is busy on most steps), in ring order
        ring, kept = [None] * T, 0
        env.reset()
        # (under a table's costs and times STEPS steps can hold fewer than T steps with a candidate: go on, up to 8x)
        for k in range(8 * STEPS if table else STEPS):
            if k >= STEPS and kept >= T:
                break
            logits = (3 * torch.randn((S, H * W, K - 1), generator=g)).to(dev)
            _, lp, _ = env.sample_actions(logits, HSEED, k)
            if bool(env.source.any()):
                env.pack_step(self.buf[kept % T])
                ring[kept % T] = (env.masks.clone().reshape(S, H * W, K), env.actions.clone(), env.source.clone(), lp, logits)
                kept += 1
            env.step()
        assert kept >= T
        self.last = (kept - 1) % T
        self.masks, self.actions, self.source = (torch.stack([r[i] for r in ring]) for i in range(3))  # [T][S]...
        self.lp, self.logits = ring[self.last][3], ring[self.last][4]
        assert env.pack_overflow() == 0 and not env.error_flags().any()
        m, a, self.names = PR.synthetic_rows(H * W, K, self.nt, seed=H * W)
        self.syn_masks, self.syn_actions = torch.from_numpy(m).to(dev), torch.from_numpy(a).to(dev)
        n = m.shape[0]
        lg = 3 * torch.randn((n, H * W, K - 1), generator=g)
        # NaN wherever the head may not look: cleared bits of candidates, every logit of the other cells
        lg[torch.from_numpy((m[:, :, 1:] == 0) | (m[:, :, :1] == 0))] = math.nan
        self.syn_logits = lg.to(dev)

    def dense(self, logits, masks, actions, g1, g2):
        """the dense kernels (the reference): logprob, entropy and gradient"""
        from microrts_amd import evaluate_actions

        lg = logits.clone().requires_grad_(True)
        lp, ent = evaluate_actions(self.env, lg, masks.contiguous(), actions.contiguous())
        (lp * g1 + ent * g2).sum().backward()
        return lp.detach(), ent.detach(), lg.grad

    def packed(self, logits, packed, index, g1, g2):
        from microrts_amd import evaluate_actions_packed

        lg = logits.clone().requires_grad_(True)
        lp, ent = evaluate_actions_packed(self.env, lg, packed, index)
        (lp * g1 + ent * g2).sum().backward()
        return lp.detach(), ent.detach(), lg.grad

    def weights(self, n):
        torch = torch_gpu()
        g = torch.Generator().manual_seed(n)
        return tuple((torch.rand(n, generator=g) + 0.5).to(self.env.device) for _ in range(2))


_CASES = {}


def _case(shape):
    if shape not in _CASES:
        _CASES[shape] = Case(shape)
    return _CASES[shape]


@pytest.fixture(scope="module", autouse=True)
def _close_table_cases():
    """the table cases' handles end with the module; the three built-in ones stay, as before"""
    yield
    for name in [n for n in _CASES if "-" in n]:
        _CASES.pop(name).env.close()


@pytest.fixture(params=CASES)
def case(request):
    return _case(request.param)


def _same(torch, got, want, tag, rows=None):
    for name, a, b in zip(("logprob", "entropy", "gradient"), got, want):
        a, b = (a, b) if rows is None else (a[rows], b[rows])
        assert torch.equal(_bits(a), _bits(b)), f"{tag}: {name} differs from the dense kernels'"


def test_format_matches_the_header(case):
    """1. the bytes pack_step writes are the bytes of the numpy packer written from include/mrts.h"""
    torch = torch_gpu()
    env = case.env
    m, a, s = (t.cpu().numpy() for t in (case.masks, case.actions, case.source))
    total = 0
    for t in range(T):
        want = PR.pack_rows(m[t], a[t], case.cap, source=s[t])
        total += int(want[:, 0].sum())
        assert np.array_equal(_np32(case.buf[t]), want), f"rollout step {t}"
    assert total > 0, "a rollout without a candidate"
    sm, sa = case.syn_masks.cpu().numpy(), case.syn_actions.cpu().numpy()
    for cap in (case.HW, 4, 1):
        out = _u32((sm.shape[0], env.packed_words(cap)), 0xDEADBEEF, env.device)
        env.pack_step(out, masks=case.syn_masks, actions=case.syn_actions)
        assert np.array_equal(_np32(out), PR.pack_rows(sm, sa, cap)), f"synthetic rows, cap {cap}"
    env.pack_overflow()
    # a view into a larger buffer at an odd word offset: only its own words are written
    big = _u32((3, sm.shape[0], env.packed_words(3)), 7, env.device)
    env.pack_step(big[1], masks=case.syn_masks, actions=case.syn_actions, cap=3)
    assert np.array_equal(_np32(big[1]), PR.pack_rows(sm, sa, 3)) and (_np32(big[0]) == 7).all() and (_np32(big[2]) == 7).all()
    env.pack_overflow()


def test_round_trip_is_the_canonical_dense_form(case):
    """2. unpack(pack(x)): the env's masks and sampled rows unchanged, junk at non-candidate cells zeroed"""
    torch = torch_gpu()
    env = case.env
    m, a = env.unpack(case.buf)
    assert torch.equal(m.reshape(T, S, case.HW, case.K), case.masks), "the env's masks are canonical"
    assert torch.equal(a.reshape(T, S, case.HW, 7), case.actions), "sampled action rows"
    idx = torch.tensor([T * S - 1, 0, 5, 5], dtype=torch.int32, device=env.device)
    m2 = torch.full((4, case.HW, case.K), 9, dtype=torch.uint8, device=env.device)
    m2, a2 = env.unpack(case.buf, index=idx, masks_out=m2)
    assert torch.equal(m2, m.reshape(T * S, case.HW, case.K)[idx.long()]) and torch.equal(a2, a[idx.long()])
    sm, sa = case.syn_masks.cpu().numpy(), case.syn_actions.cpu().numpy()
    for cap in (case.HW, 4):
        out = torch.empty((sm.shape[0], env.packed_words(cap)), dtype=torch.uint32, device=env.device)
        env.pack_step(out, masks=case.syn_masks, actions=case.syn_actions)
        m, a = env.unpack(out)
        wm, wa = PR.canonical(sm, sa, cap)
        assert np.array_equal(m.cpu().numpy().reshape(wm.shape), wm) and np.array_equal(a.cpu().numpy(), wa), f"cap {cap}"
    assert wm[:, :, 0].sum() < (sm[:, :, 0] != 0).sum() and (sa[sm[:, :, 0] == 0] != 0).any()
    env.pack_overflow()


def test_bit_equality_with_the_dense_kernels(case):
    """3. the main test: logprob, entropy and gradient equal the dense kernels' byte for byte"""
    torch = torch_gpu()
    env = case.env
    # the rollout's last step, packed with the source bits (by the rollout) and without them
    g1, g2 = case.weights(S)
    want = case.dense(case.logits, case.masks[case.last], case.actions[case.last], g1, g2)
    assert torch.isfinite(want[0]).all() and want[2].abs().sum() > 0
    _same(torch, case.packed(case.logits, case.buf[case.last], None, g1, g2), want, "rollout")
    out = torch.empty_like(case.buf[case.last])
    env.pack_step(out, masks=case.masks[case.last], actions=case.actions[case.last])
    assert torch.equal(_bits(out), _bits(case.buf[case.last])), "candidates from mask byte 0"
    _same(torch, case.packed(case.logits, out, None, g1, g2), want, "rollout, packed without the source bits")
    # the synthetic rows, cap = H*W; their NaN logits lie where neither form may look
    n = case.syn_masks.shape[0]
    g1, g2 = case.weights(n)
    want = case.dense(case.syn_logits, case.syn_masks, case.syn_actions, g1, g2)
    lp = dict(zip(case.names, want[0].tolist()))
    assert lp["none"] == 0.0 and lp["off_mask"] == -math.inf and lp["minus_one_and_huge"] == -math.inf
    assert all(math.isfinite(v) for k, v in lp.items() if k not in ("off_mask", "minus_one_and_huge")), lp
    assert torch.isfinite(want[1]).all() and torch.isfinite(want[2]).all() and want[1][1:].min() > 0
    out = torch.empty((n, env.packed_words(case.HW)), dtype=torch.uint32, device=env.device)
    env.pack_step(out, masks=case.syn_masks, actions=case.syn_actions)
    assert env.pack_overflow() == 0
    _same(torch, case.packed(case.syn_logits, out, None, g1, g2), want, "synthetic rows")
    # the canonical dense form scores the same
    m, a = env.unpack(out)
    _same(torch, case.dense(case.syn_logits, m.reshape(n, case.HW, case.K), a, g1, g2), want, "dense on unpack(pack(x))")


def test_gather_through_an_index(case):
    """4. index with repeats and a permutation == the dense call on masks[index], actions[index]"""
    torch = torch_gpu()
    env, N = case.env, T * S
    g = torch.Generator().manual_seed(5)
    idx = torch.cat([torch.randperm(N, generator=g), torch.tensor([3, 3, N - 1, 0, 3])]).to(torch.int32)
    n = idx.numel()
    logits = (3 * torch.randn((n, case.HW, case.K - 1), generator=g)).to(env.device)
    g1, g2 = case.weights(n)
    dm = case.masks.reshape(N, case.HW, case.K)[idx.long()]
    da = case.actions.reshape(N, case.HW, 7)[idx.long()]
    want = case.dense(logits, dm, da, g1, g2)
    _same(torch, case.packed(logits, case.buf, idx.to(env.device), g1, g2), want, "gather")
    # an index outside the packed rows: that row is NaN, nothing else changes
    bad = idx.clone()
    bad[1], bad[4] = -1, N
    got = case.packed(logits, case.buf, bad.to(env.device), g1, g2)
    keep = torch.ones(n, dtype=torch.bool)
    keep[[1, 4]] = False
    _same(torch, got, want, "rows beside an out-of-range index", rows=keep.to(env.device))
    for t in got:
        assert torch.isnan(t[~keep.to(env.device)]).all()


def test_overflowing_rows_are_nan_and_counted(case):
    """5. cap below a row's count: that row NaN (logprob, entropy, gradient row), the others as dense, the counter"""
    torch = torch_gpu()
    env, cap = case.env, 3
    n = case.syn_masks.shape[0]
    count = (case.syn_masks[:, :, 0] != 0).sum(1)
    over = count > cap
    assert 0 < int(over.sum()) < n and int((count == cap + 1).sum()) > 0
    g1, g2 = case.weights(n)
    want = case.dense(case.syn_logits, case.syn_masks, case.syn_actions, g1, g2)
    assert env.pack_overflow() == 0
    out = torch.empty((n, env.packed_words(cap)), dtype=torch.uint32, device=env.device)
    env.pack_step(out, masks=case.syn_masks, actions=case.syn_actions)
    got = case.packed(case.syn_logits, out, None, g1, g2)
    _same(torch, got, want, "rows within cap", rows=~over)
    for t in got:
        assert torch.isnan(t[over]).all()
    assert _np32(out)[:, 0].tolist() == count.tolist(), "word 0 keeps the true count"
    assert env.pack_overflow() == int(over.sum())
    assert env.pack_overflow() == 0


def test_determinism_and_the_first_epoch_ratio(case):
    """6. two pack and score runs give equal bytes; sample_actions' own logprob == the packed score of its rows"""
    torch = torch_gpu()
    env = case.env
    g1, g2 = case.weights(S)
    out = [torch.empty_like(case.buf[0]) for _ in range(2)]
    res = []
    for o in out:
        env.pack_step(o, masks=case.masks[case.last], actions=case.actions[case.last])
        res.append(case.packed(case.logits, o, None, g1, g2))
    assert torch.equal(_bits(out[0]), _bits(out[1]))
    _same(torch, res[0], res[1], "second run")
    assert torch.equal(_bits(res[0][0]), _bits(case.lp)), "logprob of sample_actions vs packed score of its rows"


def test_refusals():
    """7. bot-only and forward-model handles, cap outside [1, H*W], missing pointers"""
    torch = torch_gpu()
    from microrts_amd import ForwardModel, JNIGridnetVecClient, _lib

    m = "maps/4x4/basesWorkers4x4.xml"
    bots = JNIGridnetVecClient.bots(100, None, "", [m] * 2, ["PassiveAI"] * 2, ["PassiveAI"] * 2)
    fm = ForwardModel(2, m, policies=("PassiveAI", "PassiveAI"))
    dev = torch.device("cuda", 0)
    lg = torch.zeros((2, 64, 78), device=dev)
    mk = torch.zeros((2, 64, 79), dtype=torch.uint8, device=dev)
    ac = torch.zeros((2, 64, 7), dtype=torch.int32, device=dev)
    pk = _u32((2, 1 + 65 * 5), 0, dev)
    L = _lib.load()
    v = ctypes.c_int64(0)

    def calls(h, cap, n=2):
        return [L.mrts_policy_head_pack_dev(h.h, n, ptr(mk), None, ptr(ac), cap, ptr(pk), None),
                L.mrts_policy_head_unpack_dev(h.h, n, ptr(pk), 2, cap, None, ptr(mk.clone()), ptr(ac.clone()), None),
                L.mrts_policy_head_score_packed_dev(h.h, n, ptr(lg), ptr(pk), 2, cap, None, None, None, None),
                L.mrts_policy_head_grad_packed_dev(h.h, n, ptr(lg), ptr(pk), 2, cap, None, None, None, ptr(lg.clone()), None)]

    for h in (bots._h, fm._h):
        for rc in calls(h, 4):
            assert rc == -95 and "bot-only or forward-model" in L.mrts_last_error().decode()  # -ENOTSUP
        assert L.mrts_policy_head_packed_words(h.h, 4) == -95
    bots.close()
    fm.close()
    env = _case("8x8").env
    h = env._h
    assert L.mrts_policy_head_packed_words(h.h, 1) == 6 and L.mrts_policy_head_packed_words(h.h, 64) == 321
    for cap in (0, 65, -1):
        assert L.mrts_policy_head_packed_words(h.h, cap) == -22  # -EINVAL
        assert calls(h, cap) == [-22] * 4 and "cap" in L.mrts_last_error().decode()
    assert calls(h, 4, n=-1) == [-22] * 4
    # three rows of two packed rows without an index; no packed rows
    assert L.mrts_policy_head_score_packed_dev(h.h, 3, ptr(lg), ptr(pk), 2, 4, None, None, None, None) == -22
    assert L.mrts_policy_head_score_packed_dev(h.h, 2, ptr(lg), ptr(pk), 0, 4, None, None, None, None) == -22
    assert L.mrts_policy_head_pack_dev(h.h, 2, ptr(mk), None, ptr(ac), 4, None, None) == -22
    assert L.mrts_policy_head_score_packed_dev(h.h, 2, ptr(lg), None, 2, 4, None, None, None, None) == -22
    assert L.mrts_policy_head_grad_packed_dev(h.h, 2, ptr(lg), ptr(pk), 2, 4, None, None, None, None, None) == -22
    assert L.mrts_policy_head_pack_status(h.h, None) == -22 and L.mrts_policy_head_pack_status(h.h, ctypes.byref(v)) == 0
    for bad in (0, 65):
        with pytest.raises(ValueError, match="cap"):
            env.packed_buffer(2, cap=bad)
    with pytest.raises(ValueError, match="out"):
        env.pack_step(torch.zeros((S, 321), dtype=torch.int32, device=dev))
