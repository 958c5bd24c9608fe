"""bfloat16 / float16 logits through the masked policy head (mrts_policy_head_*_typed_dev, DeviceVecEnv.sample_actions,
evaluate_actions, evaluate_actions_packed) against the float32 entry points on `logits.float()`: forward outputs equal
as int32, the gradient equal to `grad32.to(dtype)` as int16.  No tolerance anywhere: a 16-bit logit converts to fp32
exactly, every step after the load is the float32 kernels', and the gradient is their value rounded once.

Cases, masks and logits: tests/policy_head_lowp_cases.py (4x4; 9x8 and 10x10 with the 55-logit table t8r5, whose cell
rows are only 2-byte aligned; 16x16; the env's masks after 50 steps and synthetic ones; logits with the largest finite
value, subnormals and -0 at set bits, NaN / inf everywhere else)."""
import ctypes

import pytest

from tests import policy_head_lowp_cases as C
from tests.gpu_support import ptr, torch_gpu

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = C.Case(name)
    return _CASES[name]


@pytest.fixture(scope="module", autouse=True)
def _close_cases():
    yield
    for name in list(_CASES):
        _CASES.pop(name).env.close()


@pytest.fixture(params=list(C.CASES))
def case(request):
    return _case(request.param)


def _equal32(torch, got, want, tag):
    for name, a, b in zip(("actions", "logprob", "entropy"), got, want):
        assert a.dtype == b.dtype and torch.equal(C.i32(a), C.i32(b)), f"{tag}: {name} differs from the float32 entry point's"


@pytest.mark.parametrize("kind", ["env", "syn"])
@pytest.mark.parametrize("name", C.DTYPES)
def test_forward_outputs_equal_the_float32_entry_points(case, name, kind):
    """1. sample (source bits and mask byte 0), score and packed score, as int32 views"""
    torch = torch_gpu()
    env, m, src = case.env, case.masks[kind], case.source[kind]
    lg, ref = case.logits(name, kind), case.ref(name, kind)
    assert lg.dtype == C.dtype_of(torch, name) and bool(torch.isfinite(ref["logprob"]).all()) and bool(torch.isfinite(ref["entropy"]).all())
    assert bool((ref["actions"] != 0).any())
    want = (ref["actions"], ref["logprob"], ref["entropy"])
    _equal32(torch, C.sample(env, lg, m, src), want, f"{case.name} {name} {kind}: sample, source bits")
    _equal32(torch, C.sample(env, lg, m, None), want, f"{case.name} {name} {kind}: sample, mask byte 0")
    _equal32(torch, (ref["actions"],) + C.score(env, lg, m, ref["actions"]), (ref["actions"],) + ref["score"],
             f"{case.name} {name} {kind}: score")
    # another seed and step draw other rows, and still the float32 call's
    l32 = lg.float()
    _equal32(torch, C.sample(env, lg, m, src, seed=5, step=3), C.sample(env, l32, m, src, seed=5, step=3), f"{case.name} {name}: seed 5")
    # MRTS_LOGITS_F32 through the typed entry points is the float32 call
    _equal32(torch, C.sample(env, l32, m, src, typed=True), want, f"{case.name} {kind}: typed float32 sample")
    _equal32(torch, (ref["actions"],) + C.score(env, l32, m, ref["actions"], typed=True), (ref["actions"],) + ref["score"],
             f"{case.name} {kind}: typed float32 score")
    p = case.packed(name, kind)
    got = C.score_packed(env, p["logits"], p["buf"], p["index"])
    _equal32(torch, (ref["actions"],) + got, (ref["actions"],) + p["score"], f"{case.name} {name} {kind}: packed score")
    nan = _nan_rows(torch, case, p)
    assert torch.isnan(got[0]).nonzero().flatten().tolist() == nan and set(nan) >= {6, 7}


def _nan_rows(torch, case, p):
    """the rows of a packed call that are NaN: an index outside the packed rows, a packed row past its cap"""
    cap = (p["buf"].shape[1] - 1) // 5
    count = p["buf"][:, 0].view(torch.int32).cpu().tolist()
    return [r for r, i in enumerate(p["index"].cpu().tolist()) if not 0 <= i < C.S or count[i] > cap]


@pytest.mark.parametrize("kind", ["env", "syn"])
@pytest.mark.parametrize("name", C.DTYPES)
def test_gradient_is_the_float32_gradient_rounded_once(case, name, kind):
    """2. dense and packed gradients equal grad32.to(dtype) as int16; every element written over the sentinel"""
    torch = torch_gpu()
    env, m = case.env, case.masks[kind]
    lg, ref = case.logits(name, kind), case.ref(name, kind)
    tag = f"{case.name} {name} {kind}"
    g32 = ref["grad"]
    assert g32.dtype == torch.float32 and bool(torch.isfinite(g32).all()) and bool((g32 != 0).any())
    got = C.grad(env, lg, m, ref["actions"], case.g_lp, case.g_ent)
    assert got.dtype == lg.dtype
    C.same_gradient(got, g32, tag + ": dense")
    dead = ~C.live_bits(m)
    assert bool((C.i16(got)[dead] == 0).all()), f"{tag}: cleared bits and non-candidate cells must be exact +0"
    # without upstream gradients (NULL = zeros): all +0 or -0 products, still every element written
    C.same_gradient(C.grad(env, lg, m, ref["actions"], None, None), C.grad(env, lg.float(), m, ref["actions"], None, None), tag + ": NULL g")
    # MRTS_LOGITS_F32 through the typed entry point is the float32 call
    t32 = C.grad(env, lg.float(), m, ref["actions"], case.g_lp, case.g_ent, typed=True)
    assert torch.equal(C.i32(t32), C.i32(g32)), f"{tag}: typed float32 gradient"
    p = case.packed(name, kind)
    nan = _nan_rows(torch, case, p)
    assert kind == "env" or case.HW <= 64 or 1 in nan, "the synthetic row with every cell a candidate overflows cap 64"
    gotp = C.grad_packed(env, p["logits"], p["buf"], p["index"], p["g_lp"], p["g_ent"])
    C.same_gradient(gotp, p["grad"], tag + ": packed", nan_rows=nan)


@pytest.mark.parametrize("name", C.DTYPES)
def test_guard_band_at_every_halfword_offset(name):
    """3. logits and gradient inside sentinel-filled buffers at each of the 8 halfword offsets of a 16-byte vector
    (9x8 with t8r5, 2 rows): the results of offset 0, and not a byte outside the gradient touched"""
    torch = torch_gpu()
    from microrts_amd import evaluate_actions

    case = _case("9x8-t8r5")
    env, dev, kind, n = case.env, case.env.device, "syn", 2
    rows = slice(2, 4)  # two rows of scattered candidates
    lg = case.logits(name, kind)[rows].contiguous()
    m, a = case.masks[kind][rows].contiguous(), case.ref(name, kind)["actions"][rows].contiguous()
    g_lp, g_ent = case.g_lp[rows].contiguous(), case.g_ent[rows].contiguous()
    buf = env.packed_buffer(1)[0][:n]
    env.pack_step(buf, masks=m, actions=a)
    numel, pad = lg.numel(), 64
    sent = C.s16(C.PATTERNS[name]["sentinel"])
    first = None
    for off in range(8):
        lbig = torch.full((numel + 2 * pad,), sent, dtype=torch.int16, device=dev)
        assert lbig.data_ptr() % 16 == 0
        lo = pad + off
        lbig[lo:lo + numel] = C.i16(lg).flatten()
        lview = lbig[lo:lo + numel].view(lg.dtype).view(lg.shape)
        assert lview.is_contiguous() and lview.data_ptr() % 16 == 2 * off
        out = {"score": C.score(env, lview, m, a), "score_packed": C.score_packed(env, lview, buf, None)}
        for which in ("grad", "grad_packed"):
            gbig = torch.full((numel + 2 * pad,), sent, dtype=torch.int16, device=dev)
            pg = ctypes.c_void_p(gbig.data_ptr() + 2 * lo)
            if which == "grad":
                C.grad(env, lview, m, a, g_lp, g_ent, p_grad=pg)
            else:
                C.grad_packed(env, lview, buf, None, g_lp, g_ent, p_grad=pg)
            assert bool((gbig[:lo] == sent).all()) and bool((gbig[lo + numel:] == sent).all()), \
                f"{name} offset {off}: {which} wrote outside its tensor"
            assert not bool((gbig[lo:lo + numel] == sent).any()), f"{name} offset {off}: {which} left elements unwritten"
            out[which] = gbig[lo:lo + numel].clone()
        # the same placement through evaluate_actions: an offset view is contiguous
        x = lview.detach().requires_grad_(True)
        lp, ent = evaluate_actions(env, x, m, a)
        ((lp * g_lp).sum() + (ent * g_ent).sum()).backward()
        out["autograd"] = (lp.detach(), ent.detach(), C.i16(x.grad).flatten())
        assert torch.equal(out["autograd"][2], out["grad"]), f"{name} offset {off}: autograd vs the C entry"
        if first is None:
            first = out
            C.same_gradient(out["grad"].view(lg.dtype).view(lg.shape), case.ref(name, kind)["grad"][rows], f"{name} offset 0")
            assert torch.equal(out["grad"], out["grad_packed"])
            continue
        for key in ("score", "score_packed", "autograd"):
            for x0, x1 in zip(first[key], out[key]):
                assert torch.equal(C.i32(x0) if x0.dtype == torch.float32 else x0, C.i32(x1) if x1.dtype == torch.float32 else x1), \
                    f"{name} offset {off}: {key} differs from offset 0"
        for key in ("grad", "grad_packed"):
            assert torch.equal(first[key], out[key]), f"{name} offset {off}: {key} differs from offset 0"


@pytest.mark.parametrize("name", C.DTYPES)
def test_autograd_returns_the_gradient_in_the_logits_type(case, name):
    """4. evaluate_actions / evaluate_actions_packed: logits.grad has the logits' type and check 2's bytes;
    sample_actions draws the rows of logits.float()"""
    torch = torch_gpu()
    from microrts_amd import evaluate_actions, evaluate_actions_packed

    env, kind = case.env, "env"
    lg, ref, m = case.logits(name, kind), case.ref(name, kind), case.masks[kind]
    x = lg.clone().requires_grad_(True)
    lp, ent = evaluate_actions(env, x, m, ref["actions"])
    assert lp.dtype == torch.float32 and ent.dtype == torch.float32
    _equal32(torch, (ref["actions"], lp.detach(), ent.detach()), (ref["actions"],) + ref["score"], f"{case.name} {name}: evaluate_actions")
    ((lp * case.g_lp).sum() + (ent * case.g_ent).sum()).backward()
    assert x.grad.dtype == lg.dtype
    C.same_gradient(x.grad, ref["grad"], f"{case.name} {name}: evaluate_actions")
    p = case.packed(name, kind)
    x = p["logits"].clone().requires_grad_(True)
    lp, ent = evaluate_actions_packed(env, x, p["buf"], p["index"])
    _equal32(torch, (ref["actions"], lp.detach(), ent.detach()), (ref["actions"],) + p["score"], f"{case.name} {name}: packed")
    nan = _nan_rows(torch, case, p)
    # (NaN rows: their upstream gradient does not matter, the kernel writes NaN)
    ((lp * p["g_lp"]).nansum() + (ent * p["g_ent"]).nansum()).backward()
    assert x.grad.dtype == lg.dtype
    keep = [r for r in range(len(p["index"])) if r not in nan]
    C.same_gradient(x.grad[keep], p["grad"][keep], f"{case.name} {name}: evaluate_actions_packed")
    assert bool(torch.isnan(x.grad[nan]).all())
    assert torch.equal(env.masks.reshape(m.shape), m)
    acts, lps, ents = env.sample_actions(lg, C.HSEED, C.HSTEP)
    assert acts is env.actions
    _equal32(torch, (acts, lps, ents), (ref["actions"], ref["logprob"], ref["entropy"]), f"{case.name} {name}: sample_actions")


def test_refusals_of_the_typed_entry_points():
    """5. value and mrts_last_error text"""
    torch = torch_gpu()
    from microrts_amd import ForwardModel, JNIGridnetVecClient, _lib

    L = _lib.load()
    case = _case("4x4")
    env, h = case.env, case.env._h
    lg = case.logits("bfloat16", "env")
    mk, ac = case.masks["env"], case.ref("bfloat16", "env")["actions"].clone()  # (the accepted sample call writes it)
    gr = torch.zeros_like(lg)
    buf = env.packed_buffer(1)[0]
    err = lambda: L.mrts_last_error().decode()  # noqa: E731
    odd = lambda t: ctypes.c_void_p(t.data_ptr() + 1)  # noqa: E731
    half = lambda t: ctypes.c_void_p(t.data_ptr() + 2)  # noqa: E731

    def calls(handle, code, pl, pg):
        """the five typed calls with one handle, type code, logits pointer and gradient pointer"""
        return [L.mrts_policy_head_sample_typed_dev(handle, code, pl, ptr(mk), None, 1, 0, ptr(ac), None, None, None),
                L.mrts_policy_head_score_typed_dev(handle, C.S, code, pl, ptr(mk), ptr(ac), None, None, None),
                L.mrts_policy_head_grad_typed_dev(handle, C.S, code, pl, ptr(mk), ptr(ac), None, None, pg, None),
                L.mrts_policy_head_score_packed_typed_dev(handle, C.S, code, pl, ptr(buf), C.S, 16, None, None, None, None),
                L.mrts_policy_head_grad_packed_typed_dev(handle, C.S, code, pl, ptr(buf), C.S, 16, None, None, None, pg, None)]

    for rc in calls(None, 1, ptr(lg), ptr(gr)):
        assert rc == -22 and err() == "null handle"
    for code in (3, -1, 1 << 20):
        for rc in calls(h.h, code, ptr(lg), ptr(gr)):
            assert rc == -22 and "logits_type" in err()
    for code in (1, 2):  # an odd address
        for rc in calls(h.h, code, odd(lg), ptr(gr)):
            assert rc == -22 and err() == "misaligned buffer"
        rcs = calls(h.h, code, ptr(lg), odd(gr))
        assert rcs[2] == -22 and rcs[4] == -22 and err() == "misaligned buffer"
    for rc in calls(h.h, 0, half(lg), ptr(gr)):  # float32 needs 4 bytes
        assert rc == -22 and err() == "misaligned buffer"
    for rc in calls(h.h, 1, None, ptr(gr)):
        assert rc == -22 and err() == "null argument"
    rcs = calls(h.h, 2, ptr(lg), None)
    assert rcs[2] == -22 and rcs[4] == -22 and err() == "null argument"
    # the same calls with nothing wrong are accepted (2-byte aligned buffers: the guard-band test)
    assert calls(h.h, 1, ptr(lg), ptr(gr)) == [0] * 5
    m = C.CASES["4x4"][0]
    bots = JNIGridnetVecClient.bots(100, None, "", [m] * 2, ["PassiveAI"] * 2, ["PassiveAI"] * 2)
    fm = ForwardModel(2, m, policies=("PassiveAI", "PassiveAI"))
    for other in (bots._h, fm._h):
        for rc in calls(other.h, 1, ptr(lg), ptr(gr)):
            assert rc == -95 and "bot-only or forward-model" in err()  # -ENOTSUP
    bots.close()
    fm.close()
    env.synchronize()
