"""Packed observation rows (include/mrts.h "Packed observation rows", mrts_obs_*_dev): what a rollout
keeps of each step's observation tensor int32 [C][H][W] — its occupied cells as two words each and planes 5.. as
bitmaps, 1 + 2 * cap + (C - 5) * ceil(H*W / 32) uint32 words a row.  DeviceVecEnv.pack_obs fills a step of an
obs_packed_buffer; onehot_packed gives the network's input of a minibatch straight from the packed rows through a
gather index, unpack_obs the int32 planes.  This module holds the argument checks (no GPU call)."""
from .policy_head import check_tensor


def default_cap(env):
    """The packed observation rows' default capacity of occupied cells: min(H*W, 128)."""
    _, H, W, _, _ = env.dims
    return min(H * W, 128)


def _bitmap_words(env):
    _, H, W, C, _ = env.dims
    return (C - 5) * ((H * W + 31) // 32)


def packed_words(env, cap=None):
    """uint32 words of a packed observation row of at most `cap` occupied cells (default min(H*W, 128))."""
    _, H, W, _, _ = env.dims
    cap = default_cap(env) if cap is None else cap
    if not isinstance(cap, int) or isinstance(cap, bool) or cap < 1 or cap > H * W:
        raise ValueError(f"cap: {cap!r}, expected an int in [1, H*W = {H * W}]")
    return 1 + 2 * cap + _bitmap_words(env)


def _cap_of(env, name, t, cap):
    """The cap a packed tensor's last dimension stands for; ValueError naming the tensor unless that is a row's words."""
    import torch

    _, H, W, _, _ = env.dims
    if not isinstance(t, torch.Tensor) or t.dim() < 2:
        raise ValueError(f"{name}: expected a uint32 tensor [rows][words]")
    words, fixed = t.shape[-1], 1 + _bitmap_words(env)
    if cap is None:
        if words < fixed + 2 or (words - fixed) % 2 or (words - fixed) // 2 > H * W:
            raise ValueError(f"{name}: {words} words is not {fixed} + 2 * cap for a cap in [1, H*W = {H * W}]")
        return (words - fixed) // 2
    if words != packed_words(env, cap):
        raise ValueError(f"{name}: {words} words, expected {packed_words(env, cap)} for cap {cap}")
    return cap


def check_pack_args(env, out, obs, cap=None):
    """The argument checks of pack_obs: out uint32 [n][words], obs int32 [n][C][H][W], both contiguous on the env's
    device.  Returns (n, cap)."""
    import torch

    _, H, W, C, _ = env.dims
    cap = _cap_of(env, "out", out, cap)
    if out.dim() != 2:
        raise ValueError(f"out: shape {tuple(out.shape)}, expected [rows][words]")
    n = out.shape[0]
    check_tensor("out", out, torch.uint32, [(n, packed_words(env, cap))], env.device)
    check_tensor("obs", obs, torch.int32, [(n, C, H, W)], env.device)
    if n * H * W >= 1 << 31:
        raise ValueError("out: rows * H*W must be below 2^31")
    return n, cap


def check_read_args(env, packed, index, cap=None):
    """The argument checks of unpack_obs / onehot_packed: packed uint32 [...][words], contiguous on the env's device;
    index (optional) int32 [rows] on it.  Returns (rows, packed rows, cap): rows is index's length, else every
    packed row."""
    import torch

    _, H, W, _, _ = env.dims
    cap = _cap_of(env, "packed", packed, cap)
    check_tensor("packed", packed, torch.uint32, [tuple(packed.shape)], env.device)
    n_packed = packed.numel() // packed.shape[-1]
    if n_packed < 1:
        raise ValueError("packed: no rows")
    rows = n_packed
    if index is not None:
        if not isinstance(index, torch.Tensor) or index.dim() != 1:
            raise ValueError("index: expected an int32 tensor [rows]")
        rows = index.shape[0]
        check_tensor("index", index, torch.int32, [(rows,)], env.device)
    if rows * H * W >= 1 << 31:
        raise ValueError(f"{'packed' if index is None else 'index'}: rows * H*W must be below 2^31")
    return rows, n_packed, cap
