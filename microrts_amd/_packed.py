"""What the argument checks of policy_head.py and obs_pack.py share (no GPU call): the pointer helper, check_tensor,
and PackedLayout — one description of a packed row (fixed words, words per item, default cap) from which both families
get their word count, the cap a tensor's last dimension stands for, and the cores of their pack and read checks."""
import ctypes


def ptr(t):
    """The tensor's device pointer for a ctypes call; None stays None (an optional argument)"""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


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


def check_rows(env, name, rows):
    """The kernels index rows * H*W cells with an int32"""
    _, H, W, _, _ = env.dims
    if rows * H * W >= 1 << 31:
        raise ValueError(f"{name}: rows * H*W must be below 2^31")


class PackedLayout:
    """A packed row is fixed(env) + cap * per_item uint32 words.  formula words the row size in a refusal (fields
    fixed, n); for_logits: the rows are read against rows of logits (the policy family), which words two refusals
    of check_read."""

    def __init__(self, per_item, cap, fixed, formula, for_logits):
        self.per_item, self.cap, self.fixed, self.formula, self.for_logits = per_item, cap, fixed, formula, for_logits

    def default_cap(self, env):
        _, H, W, _, _ = env.dims
        return min(H * W, self.cap)

    def words(self, env, cap=None):
        _, H, W, _, _ = env.dims
        cap = self.default_cap(env) if cap is None else cap
        if not isinstance(cap, int) or isinstance(cap, bool) or cap < 1 or cap > H * W:
            raise ValueError(f"cap: {cap!r}, expected an int in [1, H*W = {H * W}]")
        return self.fixed(env) + cap * self.per_item

    def cap_of(self, env, name, t, cap):
        """The cap a packed tensor's last dimension stands for; ValueError naming the tensor unless that is a row's
        words (of `cap`, when given)."""
        import torch

        _, H, W, _, _ = env.dims
        if not isinstance(t, torch.Tensor) or t.dim() < 2:
            raise ValueError(f"{name}: expected a uint32 tensor [rows][words]")
        words, fixed, n = t.shape[-1], self.fixed(env), self.per_item
        if cap is None:
            if words < fixed + n or (words - fixed) % n or (words - fixed) // n > H * W:
                raise ValueError(f"{name}: {words} words is not {self.formula.format(fixed=fixed, n=n)} for a cap in "
                                 f"[1, H*W = {H * W}]")
            return (words - fixed) // n
        if words != self.words(env, cap):
            raise ValueError(f"{name}: {words} words, expected {self.words(env, cap)} for cap {cap}")
        return cap

    def check_out(self, env, out, cap):
        """A pack call's `out`: uint32 [n][words], contiguous on the env's device.  Returns (n, cap); the caller checks
        its sources against n, then check_rows("out", n)."""
        import torch

        cap = self.cap_of(env, "out", out, cap)
        if out.dim() != 2:
            raise ValueError(f"out: shape {tuple(out.shape)}, expected [rows][words]")
        n = out.shape[0]
        check_tensor("out", out, torch.uint32, [(n, self.words(env, cap))], env.device)
        return n, cap

    def check_read(self, env, packed, index, rows=None, cap=None):
        """A read call's packed uint32 [...][words], contiguous on the env's device, and index (optional) int32 [rows]
        on it.  rows: what the caller's logits fix; None: index's length, else every packed row.  Returns (rows,
        packed rows, cap)."""
        import torch

        cap = self.cap_of(env, "packed", packed, cap)
        check_tensor("packed", packed, torch.uint32, [tuple(packed.shape)], env.device)
        n_packed = packed.numel() // packed.shape[-1]
        if n_packed < 1:
            raise ValueError("packed: no rows")
        # Three callers.  evaluate_actions_packed gives rows (its logits'), so the first block is skipped and a packed
        # tensor of another length without an index is refused.  DeviceVecEnv.unpack and the obs reads give none and
        # take rows from the index or from packed itself; an index that is no 1-d tensor is refused here by the obs
        # family in its own words, and by check_tensor below (against rows = n_packed) for unpack.
        if rows is None:
            rows = n_packed
            if isinstance(index, torch.Tensor) and index.dim() == 1:
                rows = index.shape[0]
            elif index is not None and not self.for_logits:
                raise ValueError("index: expected an int32 tensor [rows]")
        if index is not None:
            check_tensor("index", index, torch.int32, [(rows,)], env.device)
        elif n_packed != rows:
            raise ValueError(f"packed: {n_packed} rows for {rows} rows of logits (pass an index to gather)")
        # the 2^31 refusal names the logits in the policy family; the obs family names what fixed rows
        if self.for_logits:
            bound_name = "logits"
        else:
            bound_name = "packed" if index is None else "index"
        check_rows(env, bound_name, rows)
        return rows, n_packed, cap
