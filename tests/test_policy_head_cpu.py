"""The masked policy head without a GPU: the ABI lists grow together, the numpy Philox and the float64 reference
the GPU tests compare against are themselves pinned, and bad tensors are refused before any GPU call."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from microrts_amd import _lib, policy_head
from tests import oracle_py
from tests import policy_head_ref as R
from tests.python_refusal_cases import cases as refusal_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = ["mrts_policy_head_sample_dev", "mrts_policy_head_score_dev", "mrts_policy_head_grad_dev"]


def test_head_symbols_in_header_exports_and_library():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrts.h")).read(), flags=re.S)
    L = _lib.load()
    for name in HEAD:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in _lib.EXPORTS, name
        assert ctypes.cast(getattr(L, name), ctypes.c_void_p).value, name
        assert getattr(L, name).argtypes, name
    import microrts_amd

    assert microrts_amd.evaluate_actions is policy_head.evaluate_actions


@pytest.mark.parametrize("seed,slot,step", [(0x5EEDC0DE, 0, 0), (7, 3, 41), ((0xABCDEF01 << 32) | 0x12345678, 1000, 123456)])
def test_numpy_philox_reproduces_the_uniform_policy_rows(seed, slot, step):
    for H, W, K, nt in ((8, 8, 79, 7), (4, 5, 79, 7)):
        assert np.array_equal(R.uniform_rows(H, W, K, seed, slot, step, nt), oracle_py.policy_uniform(H, W, K, seed, slot, step, nt))


def test_reference_on_a_three_bit_field():
    """type field with bits 1, 2, 4 set and logits log 1, log 2, log 5: p = 1/8, 2/8, 5/8"""
    K, nt = 79, 7
    masks = torch.zeros((1, 2, K), dtype=torch.uint8)
    masks[0, 0, 0] = 1
    logits = torch.full((1, 2, K - 1), float("nan"), dtype=torch.float64)  # cleared bits and the other cell are never read
    for j, v in ((1, 1.0), (2, 2.0), (4, 5.0)):
        masks[0, 0, 1 + j] = 1
        logits[0, 0, j] = math.log(v)
    p = np.array([1, 2, 5]) / 8
    H = -(p * np.log(p)).sum()
    for k, j in enumerate((1, 2, 4)):
        a = torch.zeros((1, 2, 7), dtype=torch.int32)
        a[0, 0, 0] = j
        r = R.head_reference(logits, masks, nt, actions=a)
        assert abs(r["logprob"].item() - math.log(p[k])) < 1e-12 and abs(r["entropy"].item() - H) < 1e-12
    a[0, 0, 0] = 3  # off the mask
    assert R.head_reference(logits, masks, nt, actions=a)["logprob"].item() == -math.inf
    # the draw: the smallest set bit whose running sum exceeds u * S (boundaries at 1/8 and 3/8)
    for u0, want in ((0.0, 1), (0.1249, 1), (0.1251, 2), (0.3749, 2), (0.3751, 4), (0.99999, 4)):
        u = torch.zeros((1, 2, 7), dtype=torch.float64)
        u[0, 0, 0] = u0
        r = R.head_reference(logits, masks, nt, u=u)
        assert r["actions"][0, 0].tolist() == [want, 0, 0, 0, 0, 0, 0] and r["actions"][0, 1].abs().sum() == 0
        assert r["drawn"][0, 0].tolist() == [True] + [False] * 6 and not r["near"].any()
    u[0, 0, 0] = 0.125 + 5e-6
    assert R.head_reference(logits, masks, nt, u=u)["near"][0, 0, 0]


def test_reference_alone_stays_under_the_boundary_cap():
    """GPU test 2 leaves out components whose u lies within 1e-5 of an interior boundary and caps their share
    at 1 %: the float64 reference on the inputs that test uses (tests/test_gpu_policy_head.py's Case: six slots of
    synthetic masks and logits 3 * randn seeded with H*W, uniforms of seed 0x0123456789ABCDEF, step 17)."""
    K, nt, S = 79, 7, 6
    for HW in (16, 72, 256):
        masks = torch.from_numpy(R.synthetic_masks(S, HW, K, nt, seed=HW))
        logits = 3 * torch.randn((S, HW, K - 1), generator=torch.Generator().manual_seed(HW))
        u = torch.from_numpy(np.stack([R.head_uniforms(0x0123456789ABCDEF, s, 17, HW) for s in range(S)]))
        r = R.head_reference(logits, masks, nt, u=u)
        assert r["drawn"].sum() > 0 and r["near"].sum().item() <= 0.01 * r["drawn"].sum().item()
        # fp32 arithmetic draws the same components away from the boundaries
        r32 = R.head_reference(logits, masks, nt, u=u, dtype=torch.float32)
        keep = r["drawn"] & ~r["near"]
        assert torch.equal(r["actions"][keep], r32["actions"][keep])


def test_scorers_hand_each_entry_point_its_arguments():
    """The autograd functions of evaluate_actions and evaluate_actions_packed: on a stand-in library that records
    its calls, forward and backward of both reach their own entry points with as many arguments as _lib.SIGNATURES
    lists, an int where it has an int32 and a pointer (or None) where it has a pointer, the tensors in their places."""
    calls = []

    class Library:
        def __getattr__(self, name):
            return lambda *args: calls.append((name, args)) or 0

    env = types.SimpleNamespace(dims=(4, 4, 4, 27, 79), device=torch.device("cpu"), _s=lambda stream: None,
                                _h=types.SimpleNamespace(L=Library(), h="handle"))
    lg = torch.zeros((4, 16, 78), requires_grad=True)
    mk = torch.zeros((4, 4, 4, 79), dtype=torch.uint8)
    ac = torch.zeros((4, 16, 7), dtype=torch.int32)
    pk = torch.zeros((2, 1 + 8 * 5), dtype=torch.uint32)
    idx = torch.zeros(4, dtype=torch.int32)
    for run, names, rows in (
            (lambda: policy_head.evaluate_actions(env, lg, mk, ac), HEAD[1:], [mk, ac]),
            (lambda: policy_head.evaluate_actions_packed(env, lg, pk, idx),
             ["mrts_policy_head_score_packed_dev", "mrts_policy_head_grad_packed_dev"], [pk, 2, 8, idx]),
            (lambda: policy_head.evaluate_actions_packed(env, lg, torch.zeros((4, 41), dtype=torch.uint32)), None, None)):
        calls.clear()
        logprob, entropy = run()
        (logprob.sum() + 2 * entropy.sum()).backward()
        assert lg.grad is not None and lg.grad.shape == lg.shape
        lg.grad = None
        assert len(calls) == 2
        for name, args in calls:
            argtypes = _lib.SIGNATURES[name][0]
            assert len(args) == len(argtypes), name
            for a, t in zip(args[1:], argtypes[1:]):
                assert isinstance(a, int) if t is ctypes.c_int32 else a is None or isinstance(a, ctypes.c_void_p), (name, a, t)
        if names is None:  # no index: a null pointer in its place
            assert [c[0] for c in calls] == ["mrts_policy_head_score_packed_dev", "mrts_policy_head_grad_packed_dev"]
            assert calls[0][1][6] is None and calls[1][1][6] is None
            continue
        assert [c[0] for c in calls] == names
        want = [r.data_ptr() if isinstance(r, torch.Tensor) else r for r in rows]
        for name, args in calls:
            assert args[:2] == ("handle", 4) and args[2].value == lg.data_ptr()
            assert [a.value if isinstance(a, ctypes.c_void_p) else a for a in args[3:3 + len(rows)]] == want, name
        # the backward's three last pointers before the stream: the two incoming gradients and the one it writes
        assert all(isinstance(a, ctypes.c_void_p) for a in calls[1][1][-4:-1]) and calls[1][1][-1] is None
    calls.clear()
    policy_head.evaluate_actions(env, lg.detach(), mk, ac)  # nothing to differentiate: no backward call
    assert [c[0] for c in calls] == ["mrts_policy_head_score_dev"]


def test_bad_tensors_are_refused_before_any_gpu_call():
    env = types.SimpleNamespace(dims=(4, 4, 4, 27, 79), device=torch.device("cpu"))
    lg = torch.zeros((4, 16, 78))
    mk = torch.zeros((4, 4, 4, 79), dtype=torch.uint8)
    ac = torch.zeros((4, 16, 7), dtype=torch.int32)
    assert policy_head.check_head_args(env, lg, mk, ac) == 4
    assert policy_head.check_head_args(env, lg, mk.reshape(4, 16, 79), ac, n=4) == 4
    bad = refusal_cases()["head"]
    assert len(bad) == 10
    for name, match, call in bad:
        with pytest.raises(ValueError, match=match):
            call()
