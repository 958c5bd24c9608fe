"""Reference side of the masked policy head's tests (include/mrts.h, mrts_policy_head_*_dev) — test infrastructure.

A numpy Philox4x32-10 (the generator of the kernels' philox(), counter layouts as documented at uniformRow and at
the head's entry points), a torch reference of the head's semantics in a chosen precision (float64: the reference;
float32 on the CPU: the yardstick of what fp32 arithmetic costs, from which the GPU tests take their tolerance),
and the synthetic mask builder the CPU and GPU tests share."""
import numpy as np
import torch

UNIFORM_TAG = 0x554E4946
HEAD_TAG = 0x48454144
_M = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, seed):
    """ctr: uint32 [..., 4]; key = (seed & 2^32-1, seed >> 32).  Returns uint32 [..., 4]."""
    c = [np.asarray(ctr)[..., i].astype(np.uint64) for i in range(4)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _M, (k1 + np.uint64(0xBB67AE85)) & _M
    return np.stack(c, -1).astype(np.uint32)


def _words(seed, slot_id, step, n_cells, tag):
    ctr = np.zeros((n_cells, 4), np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = slot_id, step, np.arange(n_cells), tag
    return philox4x32_10(ctr, seed)


def uniform_rows(H, W, K, seed, slot_id, step, n_types=7):
    """mrts_policy_uniform_dev's rows of one slot from the counter layout documented at uniformRow:
    counter (slot id, step, cell, UNIFORM_TAG), ranges by multiply-shift of the words."""
    w = _words(seed, slot_id, step, H * W, UNIFORM_TAG).astype(np.uint64)
    natt = K - 23 - n_types
    a = np.zeros((H * W, 7), np.int32)
    a[:, 0] = (w[:, 0] * np.uint64(6)) >> np.uint64(32)
    for k in range(4):
        a[:, 1 + k] = (w[:, 1] >> np.uint64(2 * k)) & np.uint64(3)
    a[:, 5] = (w[:, 2] * np.uint64(n_types)) >> np.uint64(32)
    a[:, 6] = (w[:, 3] * np.uint64(natt)) >> np.uint64(32)
    return a


def head_uniforms(seed, slot_id, step, n_cells):
    """The head's uniforms of one slot: float64 [n_cells][7], field f from word f of the counters
    (slot id, step, cell, HEAD_TAG) and (.., HEAD_TAG + 1); u = (word >> 8) * 2^-24."""
    w = np.concatenate([_words(seed, slot_id, step, n_cells, HEAD_TAG), _words(seed, slot_id, step, n_cells, HEAD_TAG + 1)], 1)
    return (w[:, :7] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def fields(K, ntypes):
    """logit ranges [a, b) of the seven fields, in action-row order"""
    return [(0, 6), (6, 10), (10, 14), (14, 18), (18, 22), (22, 22 + ntypes), (22 + ntypes, K - 1)]


def head_reference(logits, masks, ntypes, actions=None, u=None, dtype=torch.float64):
    """The head's semantics on CPU tensors.  logits [n][HW][K-1] (differentiable), masks uint8 [n][HW][K];
    either actions (int [n][HW][7], scored) or u ([n][HW][7], drawn).  Returns a dict: logprob / entropy [n],
    actions [n][HW][7] (int64), drawn [n][HW][7] (component of a candidate's non-empty field), near [n][HW][7]
    (u within 1e-5 of an interior boundary of the normalised running sum)."""
    n, K = masks.shape[0], masks.shape[-1]
    masks = masks.reshape(n, -1, K) != 0
    HW = masks.shape[1]
    cand = masks[..., 0]
    lg = logits.to(dtype)
    lp = torch.zeros((n, HW), dtype=dtype)
    ent = torch.zeros((n, HW), dtype=dtype)
    acts = torch.zeros((n, HW, 7), dtype=torch.int64)
    drawn = torch.zeros((n, HW, 7), dtype=torch.bool)
    near = torch.zeros((n, HW, 7), dtype=torch.bool)
    zero, ninf = torch.zeros((), dtype=dtype), torch.full((), -float("inf"), dtype=dtype)
    for f, (a, b) in enumerate(fields(K, ntypes)):
        m = masks[..., 1 + a:1 + b] & cand[..., None]
        ne = m.any(-1)
        l = torch.where(m, lg[..., a:b], zero)
        mx = torch.where(ne, torch.where(m, l, ninf).max(-1).values, zero)
        d = l - mx[..., None]
        e = torch.where(m, torch.exp(d), zero)
        S = torch.where(ne, e.sum(-1), torch.ones((), dtype=dtype))
        logp = d - torch.log(S)[..., None]
        ent = ent + torch.where(ne, -(torch.where(m, (e / S[..., None]) * logp, zero)).sum(-1), zero)
        if u is not None:
            uf = u[..., f].to(dtype)
            run = torch.cumsum(e.detach(), -1)
            hit = m & (run > (uf * S.detach())[..., None])
            idx = torch.arange(b - a)
            first = torch.where(hit, idx, b - a).min(-1).values
            last = torch.where(m, idx, 0).max(-1).values
            comp = torch.where(first < b - a, first, last)
            interior = m & (idx < last[..., None])
            near[..., f] = ne & (interior & ((run / S.detach()[..., None] - uf[..., None]).abs() < 1e-5)).any(-1)
        else:
            comp = actions[..., f].to(torch.int64)
        inr = (comp >= 0) & (comp < b - a)
        cc = comp.clamp(0, b - a - 1)
        on = inr & torch.gather(m, -1, cc[..., None])[..., 0]
        lpf = torch.where(on, torch.gather(logp, -1, cc[..., None])[..., 0], ninf)
        lp = lp + torch.where(ne, lpf, zero)
        acts[..., f] = torch.where(ne, comp, 0) if u is not None else comp
        drawn[..., f] = ne
    return {"logprob": lp.sum(-1), "entropy": ent.sum(-1), "actions": acts, "drawn": drawn, "near": near}


def synthetic_masks(n, HW, K, ntypes, seed):
    """uint8 [n][HW][K].  Row 0 has no candidate (its other bytes are set at random all the same), row 1 every
    cell a candidate with every bit set; further rows: ~40 % candidates whose fields are, at random, empty, a
    single bit, or scattered bits — the attack window included (a ranged unit's scattered targets)."""
    g = np.random.default_rng(seed)
    m = np.zeros((n, HW, K), np.uint8)
    for r in range(n):
        kind = r % 5
        if kind == 0:
            m[r, :, 1:] = g.integers(0, 2, (HW, K - 1))
        elif kind == 1:
            m[r] = 1
        else:
            m[r, :, 0] = g.random(HW) < 0.4
            for a, b in fields(K, ntypes):
                how = g.integers(0, 3, HW)
                bits = (g.random((HW, b - a)) < 0.3).astype(np.uint8)
                bits[how == 0] = 0
                one = np.zeros((HW, b - a), np.uint8)
                one[np.arange(HW), g.integers(0, b - a, HW)] = 1
                m[r, :, 1 + a:1 + b] = np.where((how == 1)[:, None], one, bits)
    return m


def source_bits(masks):
    """mask slot 0 as the env's source bits: int32 [n][ceil(HW/32)]"""
    n, HW = masks.shape[0], masks.shape[1]
    c = np.zeros((n, (HW + 31) // 32 * 32), np.uint64)
    c[:, :HW] = masks[:, :, 0] != 0
    w = (c.reshape(n, -1, 32) << np.arange(32, dtype=np.uint64)).sum(-1)
    return w.astype(np.uint32).view(np.int32)
