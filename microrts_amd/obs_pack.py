"""Packed observation rows (include/mrts.h "Packed observation rows", mrts_obs_*_dev): what a rollout
keeps of each step's observation tensor int32 [C][H][W] — its occupied cells as two words each and planes 5.. as
bitmaps, 1 + 2 * cap + (C - 5) * ceil(H*W / 32) uint32 words a row.  DeviceVecEnv.pack_obs fills a step of an
obs_packed_buffer; onehot_packed gives the network's input of a minibatch straight from the packed rows through a
gather index, unpack_obs the int32 planes.  This module holds the argument checks (no GPU call)."""
from ._packed import PackedLayout, check_rows, check_tensor


def _bitmap_words(env):
    _, H, W, C, _ = env.dims
    return (C - 5) * ((H * W + 31) // 32)


LAYOUT = PackedLayout(per_item=2, cap=128, fixed=lambda env: 1 + _bitmap_words(env), formula="{fixed} + {n} * cap",
                      for_logits=False)


def default_cap(env):
    """The packed observation rows' default capacity of occupied cells: min(H*W, 128)."""
    return LAYOUT.default_cap(env)


def packed_words(env, cap=None):
    """uint32 words of a packed observation row of at most `cap` occupied cells (default min(H*W, 128))."""
    return LAYOUT.words(env, cap)


def check_pack_args(env, out, obs, cap=None):
    """The argument checks of pack_obs: out uint32 [n][words], obs int32 [n][C][H][W], both contiguous on the env's
    device.  Returns (n, cap)."""
    import torch

    _, H, W, C, _ = env.dims
    n, cap = LAYOUT.check_out(env, out, cap)
    check_tensor("obs", obs, torch.int32, [(n, C, H, W)], env.device)
    check_rows(env, "out", n)
    return n, cap


def check_read_args(env, packed, index, cap=None):
    """The argument checks of unpack_obs / onehot_packed: packed uint32 [...][words], contiguous on the env's device;
    index (optional) int32 [rows] on it.  Returns (rows, packed rows, cap): rows is index's length, else every
    packed row."""
    return LAYOUT.check_read(env, packed, index, cap=cap)
