"""The masked policy head (include/mrts.h, mrts_policy_head_*_dev): between a network's logits
[rows][H*W][K-1] and the action rows [rows][H*W][7].  DeviceVecEnv.sample_actions draws the rows of a rollout
step; evaluate_actions scores given rows for the update, differentiable in the logits.  A rollout keeps its masks
and action rows packed (DeviceVecEnv.packed_buffer / pack_step: the candidate cells only), and
evaluate_actions_packed scores them as they are, through an optional gather index — the same bytes out as
evaluate_actions on the dense rows.

Per candidate cell (mask slot 0 set) every field with a set mask bit is an independent masked categorical — the
GridNet factorisation of MicroRTS-Py.  An empty field adds nothing here, where MicroRTS-Py's all-masked
categorical adds the constants -log n (log-probability) and log n (entropy): PPO ratios and gradients are equal."""
from . import _lib
from ._packed import PackedLayout, check_rows, check_tensor, ptr as _p


def logits_type(logits):
    """The MRTS_LOGITS_* code of a logits tensor: float32 0, bfloat16 1, float16 2; None for any other dtype.  A
    16-bit tensor goes through the typed entry points (mrts_policy_head_*_typed_dev): its logits are converted to
    fp32 exactly as they are loaded, the forward outputs are those of `logits.float()`, and the gradient comes back
    in the logits' dtype, rounded once from the float32 value."""
    import torch

    return {torch.float32: _lib.MRTS_LOGITS_F32, torch.bfloat16: _lib.MRTS_LOGITS_BF16,
            torch.float16: _lib.MRTS_LOGITS_F16}.get(getattr(logits, "dtype", None))


def check_logits(env, logits, rows):
    """logits: float32, bfloat16 or float16 [rows][H*W][K-1], contiguous on the env's device (any other dtype is
    refused as not float32)"""
    import torch

    _, H, W, _, K = env.dims
    dtype = logits.dtype if logits_type(logits) is not None else torch.float32
    check_tensor("logits", logits, dtype, [(rows, H * W, K - 1)], env.device)


def check_head_args(env, logits, masks, actions, n=None, actions_name="actions"):
    """The argument checks of the head's calls (no GPU call): logits float32, bfloat16 or float16 [n][H*W][K-1],
    masks uint8 [n][H][W][K] (or [n][H*W][K]), actions int32 [n][H*W][7], all contiguous on the env's device.
    Returns n."""
    import torch

    _, H, W, _, K = env.dims
    if n is None:
        if not isinstance(logits, torch.Tensor) or logits.dim() != 3:
            raise ValueError("logits: expected a float32 tensor [rows][H*W][K-1]")
        n = logits.shape[0]
    check_logits(env, logits, n)
    check_tensor("masks", masks, torch.uint8, [(n, H, W, K), (n, H * W, K)], env.device)
    check_tensor(actions_name, actions, torch.int32, [(n, H * W, 7)], env.device)
    check_rows(env, "logits", n)
    return n


def _evaluate_fn():
    import torch

    class EvaluateActions(torch.autograd.Function):
        @staticmethod
        def forward(ctx, logits, masks, actions, env):
            n = logits.shape[0]
            logprob = torch.empty(n, dtype=torch.float32, device=logits.device)
            entropy = torch.empty(n, dtype=torch.float32, device=logits.device)
            h, lt = env._h, logits_type(logits)
            if lt == _lib.MRTS_LOGITS_F32:
                _lib.check(h.L.mrts_policy_head_score_dev(h.h, n, _p(logits), _p(masks), _p(actions), _p(logprob), _p(entropy),
                                                          env._s(None)))
            else:
                _lib.check(h.L.mrts_policy_head_score_typed_dev(h.h, n, lt, _p(logits), _p(masks), _p(actions), _p(logprob),
                                                                _p(entropy), env._s(None)))
            ctx.save_for_backward(logits, masks, actions)
            ctx.env = env
            ctx.set_materialize_grads(False)
            return logprob, entropy

        @staticmethod
        def backward(ctx, g_logprob, g_entropy):
            logits, masks, actions = ctx.saved_tensors
            if not ctx.needs_input_grad[0]:
                return None, None, None, None
            g = [None if t is None else t.to(torch.float32).contiguous() for t in (g_logprob, g_entropy)]
            grad = torch.empty_like(logits)  # the logits' dtype: the kernel writes it, no float32 intermediate
            h, lt = ctx.env._h, logits_type(logits)
            if lt == _lib.MRTS_LOGITS_F32:
                _lib.check(h.L.mrts_policy_head_grad_dev(h.h, logits.shape[0], _p(logits), _p(masks), _p(actions), _p(g[0]),
                                                         _p(g[1]), _p(grad), ctx.env._s(None)))
            else:
                _lib.check(h.L.mrts_policy_head_grad_typed_dev(h.h, logits.shape[0], lt, _p(logits), _p(masks), _p(actions),
                                                               _p(g[0]), _p(g[1]), _p(grad), ctx.env._s(None)))
            return grad, None, None, None

    return EvaluateActions


_EVALUATE = None


def evaluate_actions(env, logits, masks, actions):
    """(logprob, entropy), float32 [rows] each, of the given action rows under the masked categoricals of
    `logits` (float32, bfloat16 or float16 [rows][H*W][K-1]) — differentiable in `logits` (the backward is one
    mrts_policy_head_grad_dev launch on the current stream).  16-bit logits give the bytes of `logits.float()` and
    get their gradient in their own dtype, the float32 gradient rounded once (mrts_policy_head_*_typed_dev).  rows is free: an update minibatch is T x slots rows.  env: the DeviceVecEnv whose map and unit-type
    table fix H*W, K and the fields.  A component off its field's mask gives logprob -inf."""
    global _EVALUATE
    check_head_args(env, logits, masks, actions)
    if _EVALUATE is None:
        _EVALUATE = _evaluate_fn()
    return _EVALUATE.apply(logits, masks, actions, env)


CW = 5  # words per candidate of a packed row (include/mrts.h, "Packed policy rows")
LAYOUT = PackedLayout(per_item=CW, cap=64, fixed=lambda env: 1, formula="{fixed} + cap * {n}", for_logits=True)


def default_cap(env):
    """The packed rows' default candidate capacity: min(H*W, 64)."""
    return LAYOUT.default_cap(env)


def packed_words(env, cap=None):
    """uint32 words of a packed row of at most `cap` candidates (default min(H*W, 64)): 1 + cap * 5."""
    return LAYOUT.words(env, cap)


def check_pack_args(env, out, masks, actions, source=None, cap=None):
    """The argument checks of pack_step (no GPU call): out uint32 [n][words], masks uint8 [n][H][W][K] (or
    [n][H*W][K]), actions int32 [n][H*W][7], source (optional) int32 [n][ceil(H*W/32)], all contiguous on the env's
    device, words = 1 + cap * 5.  Returns (n, cap)."""
    import torch

    _, H, W, _, K = env.dims
    n, cap = LAYOUT.check_out(env, out, cap)
    check_tensor("masks", masks, torch.uint8, [(n, H, W, K), (n, H * W, K)], env.device)
    check_tensor("actions", actions, torch.int32, [(n, H * W, 7)], env.device)
    if source is not None:
        check_tensor("source", source, torch.int32, [(n, (H * W + 31) // 32)], env.device)
    check_rows(env, "out", n)
    return n, cap


def check_packed_args(env, packed, index, rows, cap=None):
    """The argument checks of the calls that read packed rows (no GPU call): packed uint32 [...][words], contiguous
    on the env's device; index (optional) int32 [rows]; without an index packed holds `rows` rows.  Returns
    (packed rows, cap)."""
    return LAYOUT.check_read(env, packed, index, rows, cap)[1:]


def _evaluate_packed_fn():
    import torch

    class EvaluateActionsPacked(torch.autograd.Function):
        @staticmethod
        def forward(ctx, logits, packed, index, env, n_packed, cap):
            n = logits.shape[0]
            logprob = torch.empty(n, dtype=torch.float32, device=logits.device)
            entropy = torch.empty(n, dtype=torch.float32, device=logits.device)
            h, lt = env._h, logits_type(logits)
            if lt == _lib.MRTS_LOGITS_F32:
                _lib.check(h.L.mrts_policy_head_score_packed_dev(h.h, n, _p(logits), _p(packed), n_packed, cap, _p(index),
                                                                 _p(logprob), _p(entropy), env._s(None)))
            else:
                _lib.check(h.L.mrts_policy_head_score_packed_typed_dev(h.h, n, lt, _p(logits), _p(packed), n_packed, cap,
                                                                       _p(index), _p(logprob), _p(entropy), env._s(None)))
            ctx.save_for_backward(logits, packed, index)
            ctx.env, ctx.n_packed, ctx.cap = env, n_packed, cap
            ctx.set_materialize_grads(False)
            return logprob, entropy

        @staticmethod
        def backward(ctx, g_logprob, g_entropy):
            logits, packed, index = ctx.saved_tensors
            if not ctx.needs_input_grad[0]:
                return None, None, None, None, None, None
            g = [None if t is None else t.to(torch.float32).contiguous() for t in (g_logprob, g_entropy)]
            grad = torch.empty_like(logits)  # the logits' dtype, written by the kernel
            h, lt = ctx.env._h, logits_type(logits)
            if lt == _lib.MRTS_LOGITS_F32:
                _lib.check(h.L.mrts_policy_head_grad_packed_dev(h.h, logits.shape[0], _p(logits), _p(packed), ctx.n_packed,
                                                                ctx.cap, _p(index), _p(g[0]), _p(g[1]), _p(grad),
                                                                ctx.env._s(None)))
            else:
                _lib.check(h.L.mrts_policy_head_grad_packed_typed_dev(h.h, logits.shape[0], lt, _p(logits), _p(packed),
                                                                      ctx.n_packed, ctx.cap, _p(index), _p(g[0]), _p(g[1]),
                                                                      _p(grad), ctx.env._s(None)))
            return grad, None, None, None, None, None

    return EvaluateActionsPacked


_EVALUATE_PACKED = None


def evaluate_actions_packed(env, logits, packed, index=None):
    """evaluate_actions on packed rows (DeviceVecEnv.pack_step): (logprob, entropy), float32 [rows], byte for byte
    what evaluate_actions gives on the dense masks and action rows that were packed, differentiable in `logits`
    (float32, bfloat16 or float16 [rows][H*W][K-1]; the backward is one launch and writes the dense gradient, in the
    logits' dtype).  packed: uint32 [N][words], or any leading shape (a [T][slots][words] rollout buffer), flattened.
    Row r is scored against
    packed row index[r] (int32 [rows] on the device, repeats allowed: a minibatch needs no copy), or against packed
    row r without an index (then N = rows).  A packed row that overflowed its cap (DeviceVecEnv.pack_overflow) and
    an index outside [0, N) give NaN for that row only."""
    global _EVALUATE_PACKED
    import torch

    if not isinstance(logits, torch.Tensor) or logits.dim() != 3:
        raise ValueError("logits: expected a float32 tensor [rows][H*W][K-1]")
    rows = logits.shape[0]
    check_logits(env, logits, rows)
    n_packed, cap = check_packed_args(env, packed, index, rows)
    if _EVALUATE_PACKED is None:
        _EVALUATE_PACKED = _evaluate_packed_fn()
    return _EVALUATE_PACKED.apply(logits, packed, index, env, n_packed, cap)
