"""The packed policy rows without a GPU: the ABI lists grow together, the documented row size, the numpy packer of
tests/policy_head_packed_ref.py on a hand-made row, and bad arguments refused before any GPU call."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from microrts_amd import DeviceVecEnv, _lib, policy_head
from tests import policy_head_packed_ref as PR
from tests.python_refusal_cases import cases as refusal_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKED = ["mrts_policy_head_pack_dev", "mrts_policy_head_unpack_dev", "mrts_policy_head_score_packed_dev",
          "mrts_policy_head_grad_packed_dev", "mrts_policy_head_packed_words", "mrts_policy_head_pack_status"]


def test_packed_symbols_in_header_exports_and_library():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrts.h")).read(), flags=re.S)
    L = _lib.load()
    for name in PACKED:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in _lib.EXPORTS, name
        assert ctypes.cast(getattr(L, name), ctypes.c_void_p).value, name
        assert getattr(L, name).argtypes, name
    import microrts_amd

    assert microrts_amd.evaluate_actions_packed is policy_head.evaluate_actions_packed
    for name in ("packed_words", "packed_buffer", "pack_step", "pack_overflow", "unpack"):
        assert callable(getattr(DeviceVecEnv, name)), name


def test_packed_words_follows_the_header():
    cw, fields, mw = PR.header_layout()
    assert (cw, mw) == (5, 3) and len(fields) == 7
    # the components' bits do not overlap, fit one word, and leave a spare value beyond every field's width
    used = 0
    for (s, b), width in zip(fields, (6, 4, 4, 4, 4, 16, 64)):
        assert used & (((1 << b) - 1) << s) == 0 and s + b <= 32 and (1 << b) - 1 >= width
        used |= ((1 << b) - 1) << s
    env = types.SimpleNamespace(dims=(4, 16, 16, 27, 79), device=torch.device("cpu"))
    assert policy_head.packed_words(env) == 1 + 64 * cw == 321  # 1,284 bytes against 256 * (79 + 28) dense
    assert DeviceVecEnv.packed_words(env, 256) == 1 + 256 * cw
    small = types.SimpleNamespace(dims=(4, 4, 4, 27, 79), device=torch.device("cpu"))
    assert policy_head.packed_words(small) == 1 + 16 * cw and policy_head.packed_words(small, 1) == 1 + cw
    bad = refusal_cases()["packed_words"]
    assert len(bad) == 6
    for name, match, call in bad:
        with pytest.raises(ValueError, match=match):
            call()


def test_numpy_packer_on_a_hand_made_row():
    K = 79
    masks = np.zeros((1, 70, K), np.uint8)
    actions = np.full((1, 70, 7), 9, np.int32)
    masks[0, 3, [0, 1, 33, 64, 78]] = [1, 255, 1, 2, 1]
    actions[0, 3] = [5, 3, -1, 7, 0, 31, 1 << 30]
    masks[0, 69, [0, 32]] = 1
    actions[0, 69] = [6, 2, 1, 0, 3, 30, 126]
    masks[0, 5, 1:] = 1  # no candidate: mask byte 0 is clear
    got = PR.pack_rows(masks, actions, 3)
    want = np.zeros((1, 16), np.uint32)
    want[0, :11] = [2, 3, 5 | 3 << 3 | 7 << 6 | 7 << 9 | 0 << 12 | 31 << 15 | 127 << 20, 1 | 2, 2, 1 | 1 << 14,
                    69, 6 | 2 << 3 | 1 << 6 | 0 << 9 | 3 << 12 | 30 << 15 | 126 << 20, 1, 1, 0]
    assert np.array_equal(got, want)
    assert np.array_equal(PR.pack_rows(masks, actions, 1)[0], np.concatenate([[2], want[0, 1:6]]).astype(np.uint32))  # overflow
    m, a = PR.canonical(masks, actions)
    assert m.sum() == 7 and m[0, 3, 1] == 1 and not m[0, 5].any()
    assert a[0, 3].tolist() == [5, 3, -1, -1, 0, -1, -1] and a[0, 69].tolist() == [6, 2, 1, 0, 3, 30, 126] and not a[0, 5].any()
    src = np.zeros((1, 3), np.int32)
    src[0, 0] = 1 << 5  # the source bits decide, not mask byte 0
    assert PR.pack_rows(masks, actions, 3, source=src)[0, :3].tolist() == [1, 5, PR.act_word([9] * 7, PR.header_layout()[1])]


def test_bad_arguments_are_refused_before_any_gpu_call():
    cpu = torch.device("cpu")
    env = types.SimpleNamespace(dims=(4, 4, 4, 27, 79), device=cpu)
    W8 = 1 + 8 * 5
    out = torch.zeros((4, W8), dtype=torch.uint32)
    mk = torch.zeros((4, 4, 4, 79), dtype=torch.uint8)
    ac = torch.zeros((4, 16, 7), dtype=torch.int32)
    src = torch.zeros((4, 1), dtype=torch.int32)
    idx = torch.zeros(4, dtype=torch.int32)
    assert policy_head.check_pack_args(env, out, mk, ac, src) == (4, 8)
    assert policy_head.check_pack_args(env, out, mk.reshape(4, 16, 79), ac, None, cap=8) == (4, 8)
    assert policy_head.check_packed_args(env, out, None, 4) == (4, 8)
    assert policy_head.check_packed_args(env, out.reshape(2, 2, W8), idx[:3], 3) == (4, 8)
    # pack_step and unpack themselves, on an object that has no handle: every refusal comes before the library is touched
    cases = refusal_cases()
    assert len(cases["pack_step"]) == 14 and len(cases["evaluate_packed"]) == 17
    for group in ("pack_step", "evaluate_packed", "unpack"):
        for name, match, call in cases[group]:
            with pytest.raises(ValueError, match=match):
                call()
