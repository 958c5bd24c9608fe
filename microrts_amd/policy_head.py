"""The masked policy head (include/mrts.h, mrts_policy_head_*_dev): between a network's logits
[rows][H*W][K-1] and the action rows [rows][H*W][7].  DeviceVecEnv.sample_actions draws the rows of a rollout
step; evaluate_actions scores given rows for the update, differentiable in the logits.

Per candidate cell (mask slot 0 set) every field with a set mask bit is an independent masked categorical — the
GridNet factorisation of MicroRTS-Py.  An empty field adds nothing here, where MicroRTS-Py's all-masked
categorical adds the constants -log n (log-probability) and log n (entropy): PPO ratios and gradients are equal."""
import ctypes

from . import _lib


def check_tensor(name, t, dtype, shapes, device):
    """ValueError naming the argument unless t is a contiguous tensor of `dtype` on `device` with one of `shapes`."""
    import torch

    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a torch tensor, got {type(t).__name__}")
    if t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if t.device != device:
        raise ValueError(f"{name}: on {t.device}, expected {device}")
    if tuple(t.shape) not in [tuple(s) for s in shapes]:
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected " + " or ".join(str(tuple(s)) for s in shapes))
    if not t.is_contiguous():
        raise ValueError(f"{name}: not contiguous")


def check_head_args(env, logits, masks, actions, n=None, actions_name="actions"):
    """The argument checks of the head's calls (no GPU call): logits float32 [n][H*W][K-1], masks uint8
    [n][H][W][K] (or [n][H*W][K]), actions int32 [n][H*W][7], all contiguous on the env's device.  Returns n."""
    import torch

    _, H, W, _, K = env.dims
    if n is None:
        if not isinstance(logits, torch.Tensor) or logits.dim() != 3:
            raise ValueError("logits: expected a float32 tensor [rows][H*W][K-1]")
        n = logits.shape[0]
    check_tensor("logits", logits, torch.float32, [(n, H * W, K - 1)], env.device)
    check_tensor("masks", masks, torch.uint8, [(n, H, W, K), (n, H * W, K)], env.device)
    check_tensor(actions_name, actions, torch.int32, [(n, H * W, 7)], env.device)
    if n * H * W >= 1 << 31:
        raise ValueError("logits: rows * H*W must be below 2^31")
    return n


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _evaluate_fn():
    import torch

    class EvaluateActions(torch.autograd.Function):
        @staticmethod
        def forward(ctx, logits, masks, actions, env):
            n = logits.shape[0]
            logprob = torch.empty(n, dtype=torch.float32, device=logits.device)
            entropy = torch.empty(n, dtype=torch.float32, device=logits.device)
            h = env._h
            _lib.check(h.L.mrts_policy_head_score_dev(h.h, n, _p(logits), _p(masks), _p(actions), _p(logprob), _p(entropy),
                                                      env._s(None)))
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
            grad = torch.empty_like(logits)
            h = ctx.env._h
            _lib.check(h.L.mrts_policy_head_grad_dev(h.h, logits.shape[0], _p(logits), _p(masks), _p(actions), _p(g[0]),
                                                     _p(g[1]), _p(grad), ctx.env._s(None)))
            return grad, None, None, None

    return EvaluateActions


_EVALUATE = None


def evaluate_actions(env, logits, masks, actions):
    """(logprob, entropy), float32 [rows] each, of the given action rows under the masked categoricals of
    `logits` — differentiable in `logits` (the backward is one mrts_policy_head_grad_dev launch on the current
    stream).  rows is free: an update minibatch is T x slots rows.  env: the DeviceVecEnv whose map and unit-type
    table fix H*W, K and the fields.  A component off its field's mask gives logprob -inf."""
    global _EVALUATE
    check_head_args(env, logits, masks, actions)
    if _EVALUATE is None:
        _EVALUATE = _evaluate_fn()
    return _EVALUATE.apply(logits, masks, actions, env)
