"""What the tests of the policy head's 16-bit logits share (a plain helper module, no tests): the element types and
their bit patterns, the logits builder, the cases, and one caller per C entry point that takes float32 logits through
the float32 export and bfloat16 / float16 logits through the typed one.

The reference of every check is the float32 entry point on `logits.float()`: forward outputs must equal it as int32,
the gradient must equal `grad32.to(dtype)` as int16 (tests/test_gpu_policy_head_lowp.py)."""
import math

import numpy as np

from tests import policy_head_ref as R, table_cases as TC
from tests.defs import SEED
from tests.gpu_support import ptr, torch_gpu

S = 6  # slots of a case's env = rows of its sample / score / gradient calls
HSEED, HSTEP = 0x0123456789ABCDEF, 17
# shape and table -> map, unit-type table of tests/table_cases.py (None: the built-in one, K = 79)
#   4x4        16 cells: less than a wave
#   9x8-t8r5   K - 1 = 55, odd: every other cell's row is only 2-byte aligned; 72 cells: an 8-cell tail chunk
#   10x10-t8r5 a row is 100 * 55 * 2 = 11,000 B = 8 mod 16: rows alternate between two offsets in the 16-byte vector
#   16x16      four chunks, the workload's shape
CASES = {"4x4": ("maps/4x4/basesWorkers4x4.xml", None), "9x8-t8r5": ("maps/NoWhereToRun9x8.xml", "t8r5"),
         "10x10-t8r5": ("maps/10x10/basesWorkers10x10.xml", "t8r5"), "16x16": ("maps/16x16/basesWorkers16x16.xml", None)}
CODES = {"float32": 0, "bfloat16": 1, "float16": 2}  # MRTS_LOGITS_* of include/mrts.h
DTYPES = ("bfloat16", "float16")
# 16-bit patterns of each type: the largest finite value, +inf, -inf, a quiet NaN, subnormals (smallest, largest, one in
# between; both signs), and a NaN the kernels never write (the sentinel a gradient buffer is pre-filled with)
PATTERNS = {
    "bfloat16": dict(max=0x7F7F, pinf=0x7F80, ninf=0xFF80, nan=0x7FC0, sub=(0x0001, 0x007F, 0x0040, 0x8001, 0x807F), sentinel=0x7FA5),
    "float16": dict(max=0x7BFF, pinf=0x7C00, ninf=0xFC00, nan=0x7E00, sub=(0x0001, 0x03FF, 0x0200, 0x8001, 0x83FF), sentinel=0x7DA5),
}
NEG_ZERO = 0x8000


def s16(x):
    """a 16-bit pattern as the int16 that holds it"""
    return x - 0x10000 if x & 0x8000 else x


def dtype_of(torch, name):
    return getattr(torch, name)


def i32(t):
    import torch

    return t.contiguous().view(torch.int32)


def i16(t):
    import torch

    return t.contiguous().view(torch.int16)


def live_bits(masks):
    """bool [n][HW][K-1]: the logits that enter the arithmetic (a set bit of a candidate cell); masks: a uint8 tensor"""
    return (masks[..., 1:] != 0) & (masks[..., :1] != 0)


def special_logits(name, masks, seed):
    """Logits of type `name` [n][HW][K-1] on the CPU for the uint8 mask tensor `masks` [n][HW][K]: 3 * randn rounded to
    the type; at set bits 5 % the largest finite value, 5 % -0 and 10 % subnormals; about one candidate cell in seven
    holds nothing but subnormals and zeros of both signs (a field whose logits differ by subnormals only: its
    probabilities show whether the conversion kept them); every logit at a cleared bit or of a cell that is no
    candidate is NaN, +inf or -inf."""
    import torch

    pat = PATTERNS[name]
    g = torch.Generator().manual_seed(seed)
    shape = (masks.shape[0], masks.shape[1], masks.shape[2] - 1)
    bits = i16((3 * torch.randn(shape, generator=g)).to(dtype_of(torch, name))).clone()
    live = live_bits(masks.cpu())
    r = torch.rand(shape, generator=g)

    def pick(values):
        v = torch.tensor([s16(x) for x in values], dtype=torch.int16)
        return v[torch.randint(0, len(values), shape, generator=g)]

    bits = torch.where(r < 0.05, torch.tensor(s16(pat["max"]), dtype=torch.int16), bits)
    bits = torch.where((r >= 0.05) & (r < 0.10), torch.tensor(s16(NEG_ZERO), dtype=torch.int16), bits)
    bits = torch.where((r >= 0.10) & (r < 0.20), pick(pat["sub"]), bits)
    tiny = torch.rand(shape[:2], generator=g)[..., None] < 0.15
    bits = torch.where(tiny, pick(pat["sub"] + (0, NEG_ZERO)), bits)
    dead = pick((pat["nan"], pat["pinf"], pat["ninf"]))
    bits = torch.where(live, bits, dead)
    return bits.view(dtype_of(torch, name))


class Case:
    """One shape and table: an env stepped 50 times; its masks with its source bits ("env") and synthetic masks
    ("syn": a row without a candidate, a row with every bit of every cell set, scattered fields).  logits(name, kind):
    the special logits of a type on the device; ref(name, kind): what the float32 entry points give on their
    `.float()` — computed once, shared by every test that compares against it."""

    def __init__(self, case):
        torch = torch_gpu()
        from microrts_amd import DeviceVecEnv, UnitTypeTable

        path, table = CASES[case]
        utt = UnitTypeTable.fromJSON(TC.utt_json(table)) if table else UnitTypeTable()
        self.name = case
        self.env = env = DeviceVecEnv(S, 0, 2000, [path] * S, seed=3, utt=utt)
        env.reset()
        for k in range(50):
            env.random_policy(SEED, k)
            env.step()
        _, H, W, _, K = env.dims
        self.HW, self.K, self.KL = H * W, K, K - 1
        self.nt = env._h.L.mrts_onehot_features(env._h.h) - 22
        assert (self.nt, K) == ((TC.TABLES[table].nt, TC.TABLES[table].K) if table else (7, 79))
        syn = R.synthetic_masks(S, H * W, K, self.nt, seed=H * W)
        self.masks = {"env": env.masks.clone().reshape(S, H * W, K), "syn": torch.from_numpy(syn).to(env.device)}
        self.source = {"env": env.source.clone(), "syn": torch.from_numpy(R.source_bits(syn)).to(env.device)}
        assert bool(self.source["env"].any()), "no candidate after 50 steps"
        g = torch.Generator().manual_seed(7 + H * W)
        self.g_lp, self.g_ent = (torch.randn(S, generator=g).to(env.device) for _ in range(2))
        self._logits, self._ref, self._packed = {}, {}, {}

    def logits(self, name, kind):
        if (name, kind) not in self._logits:
            lg = special_logits(name, self.masks[kind], seed=self.HW + CODES[name] + (100 if kind == "syn" else 0))
            self._logits[name, kind] = lg.to(self.env.device)
        return self._logits[name, kind]

    def ref(self, name, kind):
        """the float32 entry points on logits.float(): actions / logprob / entropy of a sample with the source bits,
        the score of those actions, and the float32 gradient"""
        if (name, kind) not in self._ref:
            env, m = self.env, self.masks[kind]
            l32 = self.logits(name, kind).float()
            a, lp, ent = sample(env, l32, m, self.source[kind])
            slp, sent = score(env, l32, m, a)
            self._ref[name, kind] = dict(actions=a, logprob=lp, entropy=ent, score=(slp, sent),
                                         grad=grad(env, l32, m, a, self.g_lp, self.g_ent))
        return self._ref[name, kind]

    def packed(self, name, kind):
        """The rows of `kind` packed (cap = min(H*W, 64): the synthetic row with every cell a candidate overflows it on
        every map of more than 64 cells), a gather index with repeats and two entries outside the packed rows, the
        gathered logits of type `name`, and the float32 entry points' score and gradient of them."""
        torch = torch_gpu()
        if (name, kind) not in self._packed:
            env = self.env
            a = self.ref(name, kind)["actions"]
            buf = env.packed_buffer(1)[0]
            env.pack_step(buf, masks=self.masks[kind].reshape(S, *env.dims[1:3], self.K), actions=a)
            index = torch.tensor([0, 1, 1, 3, 5, 2, S, -1], dtype=torch.int32, device=env.device)
            rows = index.clamp(0, S - 1).long()
            lg = self.logits(name, kind)[rows].contiguous()
            g = torch.Generator().manual_seed(11)
            g_lp, g_ent = (torch.randn(len(index), generator=g).to(env.device) for _ in range(2))
            l32 = lg.float()
            self._packed[name, kind] = dict(buf=buf, index=index, logits=lg, g_lp=g_lp, g_ent=g_ent,
                                            score=score_packed(env, l32, buf, index),
                                            grad=grad_packed(env, l32, buf, index, g_lp, g_ent))
        return self._packed[name, kind]


def code_of(logits):
    return CODES[str(logits.dtype).replace("torch.", "")]


def _outputs(env, n):
    torch = torch_gpu()
    return tuple(torch.full((n,), math.nan, dtype=torch.float32, device=env.device) for _ in range(2))


def sentinel_like(logits):
    """a gradient buffer of the logits' shape and type, pre-filled: NaN for float32, the type's sentinel pattern"""
    torch = torch_gpu()
    if logits.dtype == torch.float32:
        return torch.full_like(logits, math.nan)
    pat = PATTERNS[str(logits.dtype).replace("torch.", "")]
    return torch.full(logits.shape, s16(pat["sentinel"]), dtype=torch.int16, device=logits.device).view(logits.dtype)


# One caller per entry point.  float32 logits go through the float32 export unless typed=True; 16-bit logits through
# the typed export.  p_logits / p_grad: a pointer in place of the tensor's own (the guard-band placements).
def sample(env, logits, masks, source, seed=HSEED, step=HSTEP, typed=False, p_logits=None):
    torch = torch_gpu()
    from microrts_amd import _lib

    h, code = env._h, code_of(logits)
    out = torch.full((h.S, logits.shape[1], 7), -7, dtype=torch.int32, device=env.device)
    lp, ent = _outputs(env, h.S)
    pl = p_logits or ptr(logits)
    if code == 0 and not typed:
        _lib.check(h.L.mrts_policy_head_sample_dev(h.h, pl, ptr(masks), ptr(source), seed, step, ptr(out), ptr(lp), ptr(ent), env._s(None)))
    else:
        _lib.check(h.L.mrts_policy_head_sample_typed_dev(h.h, code, pl, ptr(masks), ptr(source), seed, step, ptr(out), ptr(lp),
                                                         ptr(ent), env._s(None)))
    return out, lp, ent


def score(env, logits, masks, actions, typed=False, p_logits=None):
    from microrts_amd import _lib

    h, code, n = env._h, code_of(logits), logits.shape[0]
    lp, ent = _outputs(env, n)
    pl = p_logits or ptr(logits)
    if code == 0 and not typed:
        _lib.check(h.L.mrts_policy_head_score_dev(h.h, n, pl, ptr(masks), ptr(actions), ptr(lp), ptr(ent), env._s(None)))
    else:
        _lib.check(h.L.mrts_policy_head_score_typed_dev(h.h, n, code, pl, ptr(masks), ptr(actions), ptr(lp), ptr(ent), env._s(None)))
    return lp, ent


def grad(env, logits, masks, actions, g_lp, g_ent, typed=False, p_logits=None, p_grad=None):
    """the gradient, written into a pre-filled buffer (sentinel_like) unless p_grad places it"""
    from microrts_amd import _lib

    h, code, n = env._h, code_of(logits), logits.shape[0]
    out = None if p_grad else sentinel_like(logits)
    pl, pg = p_logits or ptr(logits), p_grad or ptr(out)
    if code == 0 and not typed:
        _lib.check(h.L.mrts_policy_head_grad_dev(h.h, n, pl, ptr(masks), ptr(actions), ptr(g_lp), ptr(g_ent), pg, env._s(None)))
    else:
        _lib.check(h.L.mrts_policy_head_grad_typed_dev(h.h, n, code, pl, ptr(masks), ptr(actions), ptr(g_lp), ptr(g_ent), pg,
                                                       env._s(None)))
    return out


def score_packed(env, logits, packed, index, typed=False, p_logits=None):
    from microrts_amd import _lib

    h, code, n = env._h, code_of(logits), logits.shape[0]
    n_packed, cap = packed.shape[0], (packed.shape[1] - 1) // 5
    lp, ent = _outputs(env, n)
    pl = p_logits or ptr(logits)
    if code == 0 and not typed:
        _lib.check(h.L.mrts_policy_head_score_packed_dev(h.h, n, pl, ptr(packed), n_packed, cap, ptr(index), ptr(lp), ptr(ent),
                                                         env._s(None)))
    else:
        _lib.check(h.L.mrts_policy_head_score_packed_typed_dev(h.h, n, code, pl, ptr(packed), n_packed, cap, ptr(index), ptr(lp),
                                                               ptr(ent), env._s(None)))
    return lp, ent


def grad_packed(env, logits, packed, index, g_lp, g_ent, typed=False, p_logits=None, p_grad=None):
    from microrts_amd import _lib

    h, code, n = env._h, code_of(logits), logits.shape[0]
    n_packed, cap = packed.shape[0], (packed.shape[1] - 1) // 5
    out = None if p_grad else sentinel_like(logits)
    pl, pg = p_logits or ptr(logits), p_grad or ptr(out)
    if code == 0 and not typed:
        _lib.check(h.L.mrts_policy_head_grad_packed_dev(h.h, n, pl, ptr(packed), n_packed, cap, ptr(index), ptr(g_lp), ptr(g_ent), pg,
                                                        env._s(None)))
    else:
        _lib.check(h.L.mrts_policy_head_grad_packed_typed_dev(h.h, n, code, pl, ptr(packed), n_packed, cap, ptr(index), ptr(g_lp),
                                                              ptr(g_ent), pg, env._s(None)))
    return out


def same_gradient(got, grad32, tag, nan_rows=()):
    """got (16-bit) == grad32.to(its type) as int16; rows of nan_rows are NaN in every element of both (compared by
    position: any payload will do), no other element is NaN, and nothing of the sentinel survives"""
    import torch

    want = grad32.to(got.dtype)
    pat = PATTERNS[str(got.dtype).replace("torch.", "")]
    assert got.shape == want.shape and got.dtype != torch.float32, tag
    assert not bool((i16(got) == s16(pat["sentinel"])).any()), f"{tag}: gradient elements that were never written"
    nan = torch.zeros(got.shape, dtype=torch.bool, device=got.device)
    for r in nan_rows:
        nan[r] = True
    assert torch.equal(torch.isnan(got), nan), f"{tag}: NaN positions of the 16-bit gradient"
    assert torch.equal(torch.isnan(want), nan), f"{tag}: NaN positions of the float32 gradient"
    bad = (i16(got) != i16(want)) & ~nan
    if bool(bad.any()):
        at = bad.nonzero()[0].tolist()
        raise AssertionError(f"{tag}: gradient differs from grad32.to({got.dtype}) at {int(bad.sum())} places, first {at}: "
                             f"{got[tuple(at)].item()!r} vs {want[tuple(at)].item()!r} (float32 {grad32[tuple(at)].item()!r})")
