#!/usr/bin/env python3
"""Packed observation rows against the dense one-hot buffer they replace, at the c3 size.

Shape: 8192 slots (4096 self-play games) of basesWorkers16x16 after a 1000-step random-policy rollout; the rollout
then runs T = 32 more steps, each kept both ways: pack_obs into a packed buffer [T][slots][words] and onehot_obs into
a dense uint8 buffer [T][slots][16][16][29].  Timed on the same device and tensors, device events around batches of
calls, the median of 20 windows [min - max] after warm-up, the two sides of a leg alternating inside every repeat:

  store    pack_obs(buf[t])                      vs. onehot_obs(out=dense[t])         (a rollout step's store)
  gather   onehot_packed(buf, index=mb), B rows  vs. index_select on the dense buffer (an update's minibatch)

The two minibatches are asserted byte-equal before anything is timed.  The PyTorch gather is the baseline: a new
capability has no parent-commit number.  Also reported: the bytes pack_obs reads (from shapes) over its kernel time,
the bytes a step keeps in either form, and the largest occupied-cell count among the kept rows.

Usage (GPU box): python tools/obs_pack_bench.py [--slots 8192] [--rollout 1000] [--steps 32] [--batch 2048]
                                                [--repeats 20] [--out profiles/obs_pack.json]
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MAP = "maps/16x16/basesWorkers16x16.xml"
SEED = 0x5EEDC0DE


def timed_interleaved(torch, fns, warmup, repeats, inner):
    """ms per call of several legs: every repeat times one window of `inner` calls of each leg, in the given order"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=8192)
    ap.add_argument("--rollout", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from microrts_amd import DeviceVecEnv

    S, T, B = a.slots, a.steps, a.batch
    env = DeviceVecEnv(S, 0, 2000, [os.path.join(ROOT, MAP)] * S, seed=SEED)
    _, H, W, C, _ = env.dims
    env.reset()
    env.random_policy(SEED, 0)
    env.rollout_fused(SEED, 1, a.rollout)
    buf = env.obs_packed_buffer(T)
    buf64 = env.obs_packed_buffer(1, cap=64)
    F = env.onehot_obs().shape[-1]
    dense = torch.empty((T, S, H, W, F), dtype=torch.uint8, device=env.device)
    for t in range(T):
        env.step_fused(SEED, a.rollout + 1 + t)
        env.pack_obs(buf[t])
        env.onehot_obs(out=dense[t])
    lossy, bad = env.obs_pack_status()
    counts = (buf[..., 0].view(torch.int32) & 0x7FFFFFFF)
    g = torch.Generator().manual_seed(1)
    mb = torch.randint(0, T * S, (B,), generator=g).to(env.device)
    mb32 = mb.to(torch.int32)
    flat = dense.view(T * S, H, W, F)
    out_p = torch.empty((B, H, W, F), dtype=torch.uint8, device=env.device)
    out_d = torch.empty_like(out_p)
    env.onehot_packed(buf, index=mb32, out=out_p)
    torch.index_select(flat, 0, mb, out=out_d)
    assert lossy == 0 and torch.equal(out_p, out_d), "the packed minibatch differs from the dense one"
    assert torch.equal(env.onehot_packed(buf).view(dense.shape), dense)
    at = {"pack": 0, "dense": 0}  # the store legs walk the T steps of their buffers, as a rollout does

    def pack_leg():
        at["pack"] = (at["pack"] + 1) % T
        env.pack_obs(buf[at["pack"]])

    def dense_leg():
        at["dense"] = (at["dense"] + 1) % T
        env.onehot_obs(out=dense[at["dense"]])

    legs = {
        "pack_obs": pack_leg,
        "onehot_obs_store": dense_leg,
        "pack_obs_cap64": lambda: env.pack_obs(buf64[0]),
        "onehot_packed_gather": lambda: env.onehot_packed(buf, index=mb32, out=out_p),
        "index_select_dense": lambda: torch.index_select(flat, 0, mb, out=out_d),
    }
    r = timed_interleaved(torch, legs, 3, a.repeats, a.inner)
    read = S * C * H * W * 4
    words = buf.shape[-1]
    res = {
        "tool": "obs_pack_bench", "device": torch.cuda.get_device_name(env.device), "map": MAP, "slots": S, "rollout_steps": a.rollout,
        "T": T, "batch": B, "legs": r,
        "pack_obs_read_bytes": read,
        "pack_obs_read_GBps": read / (r["pack_obs"]["median_ms"] * 1e-3) / 1e9,
        "onehot_packed_write_bytes": B * H * W * F,
        "onehot_packed_write_GBps": B * H * W * F / (r["onehot_packed_gather"]["median_ms"] * 1e-3) / 1e9,
        "bytes_per_step": {"dense_onehot": S * H * W * F, "packed_cap128": S * words * 4, "packed_cap64": S * buf64.shape[-1] * 4,
                           "int32_planes": read},
        "occupied_cells": {"max": int(counts.max()), "mean": float(counts.float().mean()), "default_cap": (words - 1 - (C - 5) * ((H * W + 31) // 32)) // 2},
        "lossy_rows": lossy, "bad_reads": bad,
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
