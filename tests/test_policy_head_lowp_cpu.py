"""bfloat16 / float16 logits through the policy head, without a GPU: the type codes and the five typed exports are in
the header and the binding, the argument checks accept the two 16-bit types and refuse everything else in the words
they always had, and the Python calls hand float32 logits to the float32 entry points and 16-bit logits to the typed
ones with the type's code."""
import ctypes
import os
import re
import types

import pytest
import torch

from microrts_amd import _lib, device_env, policy_head
from tests import policy_head_lowp_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPED = ["mrts_policy_head_sample_typed_dev", "mrts_policy_head_score_typed_dev", "mrts_policy_head_grad_typed_dev",
         "mrts_policy_head_score_packed_typed_dev", "mrts_policy_head_grad_packed_typed_dev"]


def test_type_codes_and_typed_exports_in_header_and_binding():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mrts.h")).read(), flags=re.S)
    m = re.search(r"enum\s*\{\s*MRTS_LOGITS_F32\s*=\s*0\s*,\s*MRTS_LOGITS_BF16\s*=\s*1\s*,\s*MRTS_LOGITS_F16\s*=\s*2\s*\}", txt)
    assert m, "enum { MRTS_LOGITS_F32 = 0, MRTS_LOGITS_BF16 = 1, MRTS_LOGITS_F16 = 2 }"
    assert (_lib.MRTS_LOGITS_F32, _lib.MRTS_LOGITS_BF16, _lib.MRTS_LOGITS_F16) == (0, 1, 2)
    assert C.CODES == {"float32": 0, "bfloat16": 1, "float16": 2}
    L = _lib.load()
    for name in TYPED:
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert proto, name
        args = [a.strip() for a in proto.group(1).split(",")]
        assert "int32_t logits_type" in args and "const void* d_logits" in args, name
        assert ("void* d_grad_logits" in args) == ("grad" in name), name
        assert name in _lib.EXPORTS, name
        old = _lib.SIGNATURES[name.replace("_typed", "")][0]
        new = _lib.SIGNATURES[name][0]
        assert len(new) == len(old) + 1 and [t for t in new if t is not ctypes.c_int32] == [t for t in old if t is not ctypes.c_int32]
        assert ctypes.cast(getattr(L, name), ctypes.c_void_p).value, name
    # the float32 prototypes are what they were
    for name in TYPED:
        assert re.search(r"\bint\s+" + name.replace("_typed", "") + r"\s*\(\s*mrts_env\*\s*env,[^)]*const float\*\s*d_logits", txt), name


def _env():
    return types.SimpleNamespace(dims=(4, 4, 4, 27, 79), device=torch.device("cpu"))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_check_head_args_accepts_the_three_types(dtype):
    env = _env()
    lg = torch.zeros((4, 16, 78), dtype=dtype)
    mk = torch.zeros((4, 4, 4, 79), dtype=torch.uint8)
    ac = torch.zeros((4, 16, 7), dtype=torch.int32)
    assert policy_head.check_head_args(env, lg, mk, ac) == 4
    assert policy_head.check_head_args(env, lg, mk.reshape(4, 16, 79), ac, n=4) == 4
    assert policy_head.logits_type(lg) == {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[dtype]


def test_check_head_args_refusals_keep_their_texts():
    env = _env()
    mk = torch.zeros((4, 4, 4, 79), dtype=torch.uint8)
    ac = torch.zeros((4, 16, 7), dtype=torch.int32)
    pk = torch.zeros((4, 41), dtype=torch.uint32)
    for bad, text in ((torch.float64, "logits: dtype torch.float64, expected torch.float32"),
                      (torch.int16, "logits: dtype torch.int16, expected torch.float32"),
                      (torch.float8_e4m3fn, "logits: dtype torch.float8_e4m3fn, expected torch.float32")):
        lg = torch.zeros((4, 16, 78), dtype=bad)
        assert policy_head.logits_type(lg) is None
        with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
            policy_head.check_head_args(env, lg, mk, ac)
        with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
            policy_head.evaluate_actions_packed(env, lg, pk)
    for dtype in (torch.bfloat16, torch.float16):
        with pytest.raises(ValueError, match=re.escape("logits: shape (4, 16, 77), expected (4, 16, 78)")):
            policy_head.check_head_args(env, torch.zeros((4, 16, 77), dtype=dtype), mk, ac)
        with pytest.raises(ValueError, match=re.escape("logits: shape (3, 16, 78), expected (4, 16, 78)")):
            policy_head.check_head_args(env, torch.zeros((3, 16, 78), dtype=dtype), mk, ac, n=4)
        with pytest.raises(ValueError, match="^logits: not contiguous$"):
            policy_head.check_head_args(env, torch.zeros((4, 16, 156), dtype=dtype)[:, :, ::2], mk, ac)
        with pytest.raises(ValueError, match="^logits: not contiguous$"):
            policy_head.evaluate_actions_packed(env, torch.zeros((4, 16, 156), dtype=dtype)[:, :, ::2], pk)
        with pytest.raises(ValueError, match=re.escape("logits: expected a float32 tensor [rows][H*W][K-1]")):
            policy_head.check_head_args(env, torch.zeros((16, 78), dtype=dtype), mk, ac)


class _Library:
    """a stand-in library that records its calls"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *args: self.calls.append((name, args)) or 0


def _arguments_fit(name, args):
    argtypes = _lib.SIGNATURES[name][0]
    assert len(args) == len(argtypes), name
    for a, t in zip(args[1:], argtypes[1:]):
        ok = isinstance(a, int) if t in (ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint64) else a is None or isinstance(a, ctypes.c_void_p)
        assert ok, (name, a, t)


TYPES = [(torch.float32, 0), (torch.bfloat16, 1), (torch.float16, 2)]


def test_scorers_pick_the_entry_point_by_the_logits_type():
    """forward and backward of evaluate_actions and evaluate_actions_packed: float32 reaches the float32 entry points
    with their argument lists, a 16-bit type the typed ones with its code after the row count; as many arguments as
    _lib.SIGNATURES lists; the gradient the backward hands out has the logits' type"""
    for dtype, code in TYPES:
        _scorers(dtype, code)


def _scorers(dtype, code):
    lib = _Library()
    env = types.SimpleNamespace(dims=(4, 4, 4, 27, 79), device=torch.device("cpu"), _s=lambda stream: None,
                                _h=types.SimpleNamespace(L=lib, h="handle"))
    lg = torch.zeros((4, 16, 78), dtype=dtype, requires_grad=True)
    mk = torch.zeros((4, 4, 4, 79), dtype=torch.uint8)
    ac = torch.zeros((4, 16, 7), dtype=torch.int32)
    pk = torch.zeros((2, 1 + 8 * 5), dtype=torch.uint32)
    idx = torch.zeros(4, dtype=torch.int32)
    sfx = "_dev" if code == 0 else "_typed_dev"
    for run, names, rest in (
            (lambda: policy_head.evaluate_actions(env, lg, mk, ac), ["mrts_policy_head_score", "mrts_policy_head_grad"], [mk, ac]),
            (lambda: policy_head.evaluate_actions_packed(env, lg, pk, idx),
             ["mrts_policy_head_score_packed", "mrts_policy_head_grad_packed"], [pk, 2, 8, idx])):
        lib.calls.clear()
        logprob, entropy = run()
        assert logprob.dtype == torch.float32 and entropy.dtype == torch.float32
        (logprob.sum() + 2 * entropy.sum()).backward()
        assert lg.grad is not None and lg.grad.shape == lg.shape and lg.grad.dtype == dtype
        lg.grad = None
        assert [c[0] for c in lib.calls] == [n + sfx for n in names]
        want = [r.data_ptr() if isinstance(r, torch.Tensor) else r for r in rest]
        for name, args in lib.calls:
            _arguments_fit(name, args)
            assert args[:2] == ("handle", 4)
            at = 2
            if code:
                assert args[2] == code and not isinstance(args[2], bool)
                at = 3
            assert args[at].value == lg.data_ptr()
            assert [a.value if isinstance(a, ctypes.c_void_p) else a for a in args[at + 1:at + 1 + len(rest)]] == want, name
        # the backward's three last pointers before the stream: the two incoming gradients and the one it writes
        assert all(isinstance(a, ctypes.c_void_p) for a in lib.calls[1][1][-4:-1]) and lib.calls[1][1][-1] is None


def test_sample_actions_picks_the_entry_point_by_the_logits_type():
    for dtype, code in TYPES:
        _sampler(dtype, code)


def _sampler(dtype, code):
    lib = _Library()
    T = torch
    env = types.SimpleNamespace(dims=(4, 4, 4, 27, 79), device=T.device("cpu"), torch=T, _s=lambda stream: None,
                                _p=policy_head._p, _h=types.SimpleNamespace(L=lib, h="handle", S=4), _policy_stamp=lambda out: None,
                                masks=T.zeros((4, 4, 4, 79), dtype=T.uint8), source=T.zeros((4, 1), dtype=T.int32),
                                actions=T.zeros((4, 16, 7), dtype=T.int32))
    lg = T.zeros((4, 16, 78), dtype=dtype)
    out, logprob, entropy = device_env.DeviceVecEnv.sample_actions(env, lg, 99, 5)
    assert out is env.actions and logprob.dtype == T.float32 and entropy.dtype == T.float32
    (name, args), = lib.calls
    assert name == ("mrts_policy_head_sample_dev" if code == 0 else "mrts_policy_head_sample_typed_dev")
    _arguments_fit(name, args)
    at = 1
    if code:
        assert args[1] == code
        at = 2
    assert args[0] == "handle" and args[at].value == lg.data_ptr()
    assert [a.value for a in args[at + 1:at + 3]] == [env.masks.data_ptr(), env.source.data_ptr()] and args[at + 3:at + 5] == (99, 5)
    assert args[at + 5].value == env.actions.data_ptr() and args[-1] is None
    with pytest.raises(ValueError, match=re.escape("logits: dtype torch.float64, expected torch.float32")):
        device_env.DeviceVecEnv.sample_actions(env, lg.double(), 99, 5)
