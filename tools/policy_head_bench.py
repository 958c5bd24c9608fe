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

Usage (GPU box): python tools/policy_head_bench.py [--slots 4096] [--rollout 1000] [--repeats 20]
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


def sectors(np, starts, length):
    """distinct 32-byte sectors touched by byte ranges [start, start + length)"""
    first, last = starts // 32, (starts + length - 1) // 32
    span = int((last - first).max()) + 1
    s = np.concatenate([np.minimum(first + k, last) for k in range(span)])
    return int(np.unique(s).size)


def main():
    import numpy as np
    import torch

    from microrts_amd import DeviceVecEnv, evaluate_actions

    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=4096)
    ap.add_argument("--rollout", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    a = ap.parse_args()
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
    cand = masks[..., 0] != 0
    mbool = (masks[..., 1:] != 0) & cand[..., None]  # MicroRTS-Py masks every field of a cell without a unit
    n_cand = int(cand.sum())

    # the kernels
    acts, lp_k, ent_k = env.sample_actions(logits, SEED, 7)
    acts = acts.clone()
    g_lp, g_ent = torch.randn(S, device=dev), torch.randn(S, device=dev)
    lk = logits.clone().requires_grad_(True)

    def k_sample():
        env.sample_actions(logits, SEED, 7)

    def k_update():
        lk.grad = None
        lp, ent = evaluate_actions(env, lk, masks, acts)
        ((lp * g_lp).sum() + (ent * g_ent).sum()).backward()

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
    k_update()
    t_update()
    d_grad = float((lk.grad - lt.grad).abs().max())
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
        "logit_rows": n_cand * KL * 4, "logit_sector_bytes": 32 * sectors(np, cells * KL * 4, KL * 4),
    }
    dense = S * HW * KL * 4
    res.update({
        "shape": {"slots": S, "map": MAP, "cells": HW, "logits_per_cell": KL, "rollout_steps": a.rollout},
        "candidate_cells": n_cand, "candidate_density": n_cand / (S * HW),
        "sample_bytes_read": read,
        "sample_sector_bytes_read": read["source_bits"] + read["mask_sector_bytes"] + read["logit_sector_bytes"],
        "dense_logit_bytes": dense,
        "sample_read_share_of_dense": (read["source_bits"] + read["mask_sector_bytes"] + read["logit_sector_bytes"]) / dense,
        "check": {"logprob_max_abs_diff": d_lp, "entropy_max_abs_diff": d_ent, "grad_max_abs_diff": d_grad, "logprob_scale": scale},
    })
    print(json.dumps(res))
    env.close()


if __name__ == "__main__":
    main()
