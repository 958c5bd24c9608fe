#!/usr/bin/env python3
"""The masked policy head against a plain-PyTorch masked-categorical head, on the c3 map.

Shape: 4096 slots (2048 self-play games) of basesWorkers16x16 — logits float32 [4096][256][78], 327 MB — on the
masks a 1000-step random-policy rollout leaves.  Timed, on the same device and the same tensors:

  sample   DeviceVecEnv.sample_actions (one launch, driven by the source bits)
           vs. per field where(mask, logit, -1e8) -> softmax -> multinomial -> gather -> entropy over every cell
           (MicroRTS-Py's GridNet head: dense, all cells)
  update   evaluate_actions + backward (score launch + gradient launch)
           vs. the same PyTorch head's log-probability / entropy of given actions + autograd backward

Device events on the stream around batches of calls, after warm-up; median / min / max over the repeats.  The
PyTorch head is the baseline: a new capability has no parent-commit number.  Also reported: the candidate density
and the bytes the sampling kernel reads (the 32-byte sectors its loads touch) against the dense logits.  The
kernel's log-probability is checked against the PyTorch head's on the kernel's own actions (they differ by the
empty fields' and non-candidate cells' constants, sum of -log n, which the check adds back).

--packed adds the packed rollout rows on the same masks and actions: pack_step (one launch, with the
source bits and from mask byte 0), and evaluate_actions_packed + backward against evaluate_actions + backward.  The
dense update is timed twice, before and after the packed one in every repeat (window order dense, packed, dense): the
difference of the two dense medians is the noise floor the packed figure is read against.  The same three windows are
timed once more with the two launches alone (score, gradient; the C entry points), where the host's PyTorch ops
of the loss do not bound the figure.  The packed results are
checked to equal the dense ones byte for byte.  Also the bytes per step a rollout keeps in either form.

--dtype bfloat16 / float16 gives the kernels' legs (dense and --packed) the logits in that type: the
typed entry points, the gradient written in the type.  The built-in check is then bit equality: action rows,
log-probability and entropy equal the float32 entry points' on logits.float() as int32, the gradient equals their
gradient cast to the type as int16; the PyTorch head (float32, on logits.float()) stays the baseline and is still
checked against the float32 entry points.  --cast-from bfloat16 / float16 (with --dtype float32) is what a learner pays
without that: the network's logits are 16-bit, and every timed kernel leg includes logits.float() and, in the update,
autograd's cast of the float32 gradient back.  The same 16-bit values feed both, so a --cast-from run of one library
and a --dtype run of another compare like for like.

Usage (GPU box): python tools/policy_head_bench.py [--slots 4096] [--rollout 1000] [--repeats 20] [--packed]
                 [--dtype float32|bfloat16|float16] [--cast-from bfloat16|float16]
Prints one JSON line.
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAP = "maps/16x16/basesWorkers16x16.xml"
SEED = 0x5EEDC0DE


def fields(K, ntypes):
    return [(0, 6), (6, 10), (10, 14), (14, 18), (18, 22), (22, 22 + ntypes), (22 + ntypes, K - 1)]


def torch_head(torch, logits, masks, fl, actions=None):
    """MicroRTS-Py's head in plain PyTorch: every cell, every field a categorical over where(mask, logit, -1e8).
    masks: bool [S][HW][K-1].  Returns (actions int64 [S][HW][7], logprob [S], entropy [S])."""
    S, HW, _ = logits.shape
    lp = torch.zeros((S, HW), dtype=torch.float32, device=logits.device)
    ent = torch.zeros_like(lp)
    out = []
    for f, (a, b) in enumerate(fl):
        lg = torch.where(masks[..., a:b], logits[..., a:b], torch.tensor(-1e8, device=logits.device))
        logp = torch.log_softmax(lg, -1)
        p = logp.exp()
        if actions is None:
            comp = torch.multinomial(p.reshape(-1, b - a), 1).reshape(S, HW)
        else:
            comp = actions[..., f]
        out.append(comp)
        lp = lp + torch.gather(logp, -1, comp[..., None])[..., 0]
        ent = ent - (p * logp).sum(-1)
    return torch.stack(out, -1), lp.sum(-1), ent.sum(-1)


def timed(torch, fn, warmup, repeats, inner):
    """ms per call: events around `inner` calls, `repeats` times, after `warmup` batches"""
    for _ in range(warmup):
        for _ in range(inner):
            fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "calls_per_window": inner, "windows": repeats}


def timed_interleaved(torch, fns, warmup, repeats, inner):
    """timed() for several legs at once: every repeat times one window of each leg, in the given order"""
    for _ in range(warmup):
        for fn in fns.values():
            for _ in range(inner):
                fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1) / inner)
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "calls_per_window": inner, "windows": repeats}
            for k, v in ts.items()}


def sectors(np, starts, length):
    """distinct 32-byte sectors touched by byte ranges [start, start + length)"""
    first, last = starts // 32, (starts + length - 1) // 32
    span = int((last - first).max()) + 1
    s = np.concatenate([np.minimum(first + k, last) for k in range(span)])
    return int(np.unique(s).size)


def packed_leg(torch, env, evaluate_actions, evaluate_actions_packed, a, logits, masks, acts, g_lp, g_ent, k_update, lk, feed):
    """the --packed figures; env.actions holds `acts` (sample_actions wrote them) and env.source the masks' bits.
    logits: the network's; feed(logits): what the kernels get (the cast of --cast-from, else the tensor itself)"""
    S, HW, K = masks.shape
    assert torch.equal(env.actions, acts)
    buf = env.packed_buffer(1)
    cap = (buf.shape[-1] - 1) // 5
    env.pack_step(buf[0])
    other = torch.empty_like(buf[0])
    env.pack_step(other, masks=masks, actions=acts)  # candidates from mask byte 0
    assert torch.equal(buf[0].view(torch.int32), other.view(torch.int32))
    overflow = env.pack_overflow()
    lp_ = logits.clone().requires_grad_(True)
    rows = buf[0]  # (a view: made once, as the dense leg's tensors are)

    def p_update():
        lp_.grad = None
        lp, ent = evaluate_actions_packed(env, feed(lp_), rows)
        ((lp * g_lp).sum() + (ent * g_ent).sum()).backward()
        return lp, ent

    with torch.no_grad():
        d = evaluate_actions(env, feed(logits), masks, acts)
    p = p_update()
    k_update()
    i32 = torch.int32
    equal = all(torch.equal(x.detach().view(i32), y.view(i32)) for x, y in zip(p, d)) and torch.equal(lp_.grad.view(i32), lk.grad.view(i32))
    assert equal or overflow, "packed score / gradient differ from the dense ones"
    t = timed_interleaved(torch, {"update_dense_a": k_update, "update_packed": p_update, "update_dense_b": k_update}, a.warmup, a.repeats, 5)
    # the two launches alone (score, gradient), without autograd and the loss's PyTorch ops around them
    from microrts_amd import _lib

    h, P = env._h, env._p
    logits = feed(logits)  # the launches alone: no cast inside the window
    lp, ent, grad = torch.empty(S, device=env.device), torch.empty(S, device=env.device), torch.empty_like(logits)
    code = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}[logits.dtype]  # MRTS_LOGITS_*

    def d_launches():
        if code == 0:
            _lib.check(h.L.mrts_policy_head_score_dev(h.h, S, P(logits), P(masks), P(acts), P(lp), P(ent), env._s(None)))
            _lib.check(h.L.mrts_policy_head_grad_dev(h.h, S, P(logits), P(masks), P(acts), P(g_lp), P(g_ent), P(grad), env._s(None)))
        else:
            _lib.check(h.L.mrts_policy_head_score_typed_dev(h.h, S, code, P(logits), P(masks), P(acts), P(lp), P(ent), env._s(None)))
            _lib.check(h.L.mrts_policy_head_grad_typed_dev(h.h, S, code, P(logits), P(masks), P(acts), P(g_lp), P(g_ent), P(grad),
                                                           env._s(None)))

    def p_launches():
        if code == 0:
            _lib.check(h.L.mrts_policy_head_score_packed_dev(h.h, S, P(logits), P(buf), S, cap, None, P(lp), P(ent), env._s(None)))
            _lib.check(h.L.mrts_policy_head_grad_packed_dev(h.h, S, P(logits), P(buf), S, cap, None, P(g_lp), P(g_ent), P(grad),
                                                            env._s(None)))
        else:
            _lib.check(h.L.mrts_policy_head_score_packed_typed_dev(h.h, S, code, P(logits), P(buf), S, cap, None, P(lp), P(ent),
                                                                   env._s(None)))
            _lib.check(h.L.mrts_policy_head_grad_packed_typed_dev(h.h, S, code, P(logits), P(buf), S, cap, None, P(g_lp), P(g_ent),
                                                                  P(grad), env._s(None)))

    t.update(timed_interleaved(torch, {"launches_dense_a": d_launches, "launches_packed": p_launches, "launches_dense_b": d_launches},
                               a.warmup, a.repeats, 20))
    t.update(timed_interleaved(torch, {"pack_step": lambda: env.pack_step(buf[0]),
                                       "pack_step_mask_byte_0": lambda: env.pack_step(other, masks=masks, actions=acts)},
                               a.warmup, a.repeats, 50))
    env.pack_overflow()
    da, db, pk = (t[k]["median_ms"] for k in ("update_dense_a", "update_dense_b", "update_packed"))
    t.update({
        "cap": cap, "overflow_rows": overflow, "bit_identical_to_dense": bool(equal),
        "dense_bytes_per_step": S * HW * (K + 28), "packed_bytes_per_step": S * buf.shape[-1] * 4,
        "bytes_ratio": HW * (K + 28) / (buf.shape[-1] * 4),
        "noise_floor_ms": abs(da - db), "packed_minus_dense_ms": pk - (da + db) / 2,
        "launches_noise_floor_ms": abs(t["launches_dense_a"]["median_ms"] - t["launches_dense_b"]["median_ms"]),
        "launches_packed_minus_dense_ms": t["launches_packed"]["median_ms"]
        - (t["launches_dense_a"]["median_ms"] + t["launches_dense_b"]["median_ms"]) / 2,
    })
    return t


def main():
    import numpy as np
    import torch

    from microrts_amd import DeviceVecEnv, evaluate_actions, evaluate_actions_packed

    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--rollout", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--packed", action="store_true", help="also the packed rollout rows against the dense update")
    ap.add_argument("--dtype", choices=["float32", "bfloat16", "float16"], default="float32", help="the logits the kernels get")
    ap.add_argument("--cast-from", choices=["bfloat16", "float16"], default=None,
                    help="with --dtype float32: the network's logits have this type, the timed kernel legs include the casts")
    a = ap.parse_args()
    if a.cast_from and a.dtype != "float32":
        raise SystemExit("--cast-from goes with --dtype float32")
    if not torch.cuda.is_available():
        raise SystemExit("policy_head_bench needs an MI355X")
    S = a.slots
    env = DeviceVecEnv(S, 0, 2000, [os.path.join(ROOT, MAP)] * S, seed=SEED)
    _, H, W, _, K = env.dims
    HW, KL, nt = H * W, K - 1, 7
    fl = fields(K, nt)
    env.reset()
    env.random_policy(SEED, 0)
    env.rollout_fused(SEED, 1, a.rollout)
    env.synchronize()
    dev = env.device
    masks = env.masks.reshape(S, HW, K)
    logits = 3 * torch.randn((S, HW, KL), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    # net: the network's logits; feed(net): what the kernels get; logits: their float32 values (the PyTorch head's input)
    net = logits.to(getattr(torch, a.cast_from or a.dtype))
    feed = (lambda t: t.float()) if a.cast_from else (lambda t: t)
    logits = net.float()
    esize = feed(net).element_size()
    cand = masks[..., 0] != 0
    mbool = (masks[..., 1:] != 0) & cand[..., None]  # MicroRTS-Py masks every field of a cell without a unit
    n_cand = int(cand.sum())

    # the kernels
    acts, lp_k, ent_k = env.sample_actions(logits, SEED, 7)
    acts = acts.clone()
    g_lp, g_ent = torch.randn(S, device=dev), torch.randn(S, device=dev)
    lk = net.clone().requires_grad_(True)

    def k_sample():
        env.sample_actions(feed(net), SEED, 7)

    def k_update():
        lk.grad = None
        lp, ent = evaluate_actions(env, feed(lk), masks, acts)
        ((lp * g_lp).sum() + (ent * g_ent).sum()).backward()

    # the float32 entry points on the float32 values: what the PyTorch head is checked against, and what 16-bit
    # logits must reproduce bit for bit
    l32 = logits.clone().requires_grad_(True)
    lp32, ent32 = evaluate_actions(env, l32, masks, acts)
    ((lp32 * g_lp).sum() + (ent32 * g_ent).sum()).backward()
    bits = None
    if a.dtype != "float32":
        i32, i16 = torch.int32, torch.int16
        acts16, lp16, ent16 = env.sample_actions(net, SEED, 7)
        with torch.no_grad():
            s16 = evaluate_actions(env, net, masks, acts)
        k_update()
        bits = {
            "sample_equal": bool(torch.equal(acts16, acts) and torch.equal(lp16.view(i32), lp_k.view(i32))
                                 and torch.equal(ent16.view(i32), ent_k.view(i32))),
            "score_equal": bool(torch.equal(s16[0].view(i32), lp32.detach().view(i32)) and torch.equal(s16[1].view(i32), ent32.detach().view(i32))),
            "grad_equal": bool(lk.grad.dtype == net.dtype and torch.equal(lk.grad.view(i16), l32.grad.to(net.dtype).view(i16))),
        }
        assert all(bits.values()), bits

    # the PyTorch head on the same tensors
    a64 = acts.long()
    lt = logits.clone().requires_grad_(True)

    def t_sample():
        with torch.no_grad():
            torch_head(torch, logits, mbool, fl)

    def t_update():
        lt.grad = None
        _, lp, ent = torch_head(torch, lt, mbool, fl, a64)
        ((lp * g_lp).sum() + (ent * g_ent).sum()).backward()

    # same results: the PyTorch head's log-probability of the kernel's actions minus its constants (-log n per
    # empty field of a candidate and per field of every other cell), and the gradients where both are defined
    with torch.no_grad():
        _, lp_t, ent_t = torch_head(torch, logits, mbool, fl, a64)
        const = sum((~mbool[..., lo:hi].any(-1)).sum(-1).float() * math.log(hi - lo) for lo, hi in fl)
        d_lp = float((lp_t + const - lp_k).abs().max())
        d_ent = float((ent_t - const - ent_k).abs().max())
    t_update()
    d_grad = float((l32.grad - lt.grad).abs().max())
    scale = float(lp_t.abs().max())
    assert d_lp <= 1e-5 * scale + 1e-2 and d_ent <= 1e-5 * scale + 1e-2 and d_grad <= 1e-4, (d_lp, d_ent, d_grad)

    res = {
        "sample_kernel": timed(torch, k_sample, a.warmup, a.repeats, 50),
        "sample_torch": timed(torch, t_sample, a.warmup, a.repeats, 1),
        "update_kernel": timed(torch, k_update, a.warmup, a.repeats, 5),
        "update_torch": timed(torch, t_update, a.warmup, a.repeats, 1),
    }
    res["sample_speedup"] = res["sample_torch"]["median_ms"] / res["sample_kernel"]["median_ms"]
    res["update_speedup"] = res["update_torch"]["median_ms"] / res["update_kernel"]["median_ms"]

    # bytes the sampling kernel reads: the source bits, and per candidate cell its mask record and logit row
    cells = cand.reshape(-1).nonzero()[:, 0].cpu().numpy().astype(np.int64)
    read = {
        "source_bits": S * ((HW + 31) // 32) * 4,
        "mask_records": n_cand * K, "mask_sector_bytes": 32 * sectors(np, cells * K, K),
        "logit_rows": n_cand * KL * esize, "logit_sector_bytes": 32 * sectors(np, cells * KL * esize, KL * esize),
    }
    dense = S * HW * KL * esize
    res.update({
        "shape": {"slots": S, "map": MAP, "cells": HW, "logits_per_cell": KL, "rollout_steps": a.rollout},
        "candidate_cells": n_cand, "candidate_density": n_cand / (S * HW),
        "sample_bytes_read": read,
        "sample_sector_bytes_read": read["source_bits"] + read["mask_sector_bytes"] + read["logit_sector_bytes"],
        "dtype": a.dtype, "cast_from": a.cast_from, "bit_equal_to_float32": bits,
        "dense_logit_bytes": dense, "gradient_bytes_written": dense,
        "sample_read_share_of_dense": (read["source_bits"] + read["mask_sector_bytes"] + read["logit_sector_bytes"]) / dense,
        "check": {"logprob_max_abs_diff": d_lp, "entropy_max_abs_diff": d_ent, "grad_max_abs_diff": d_grad, "logprob_scale": scale},
    })
    if a.packed:
        res["packed"] = packed_leg(torch, env, evaluate_actions, evaluate_actions_packed, a, net, masks, acts, g_lp, g_ent, k_update, lk,
                                   feed)
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
