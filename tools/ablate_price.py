#!/usr/bin/env python3
"""Diagnostic: marginal cost of each k_env phase, priced by running it twice (libmrts_ablate.so,
built with `make -C microrts_amd/csrc ablate`; a bit of g_ablate doubles its phase idempotently, so the
game dynamics are unchanged — tests/test_gpu_ablate.py holds every such bit, set at once, against the
product library).  The c3 workload is checkpointed after the burn-in; every variant
restores it, runs 5 untimed steps and times the same 100 fused steps (native rollout, HIP events);
variants are interleaved with baseline runs, 5 rounds, medians.  Prints one JSON line per phase:
the extra microseconds per step of its second copy ("SKIP x": negative = what x costs)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from tools import ablate_table  # noqa: E402

L, PHASES = ablate_table.load()  # the rows of microrts_amd/csrc/mrts_ablate.h: bits, kinds and the names printed here
from microrts_amd import DeviceVecEnv  # noqa: E402

SEED = 0x5EEDC0DE


def main():
    import numpy as np

    E = int(os.environ.get("E", 4096))
    MAP = os.environ.get("MAP", "maps/16x16/basesWorkers16x16.xml")
    burn = int(os.environ.get("BURNIN", 1000))
    K = 100
    PO = os.environ.get("PO", "0") == "1"
    UNI = os.environ.get("UNIFORM", "0") == "1"  # c2: fused unmasked uniform rows, no masks
    env = DeviceVecEnv(2 * E, 0, 2000, [os.path.join(ROOT, MAP)] * (2 * E), seed=SEED, partial_obs=PO,
                       max_units=int(os.environ.get("MAXU", 0)), with_masks=not UNI)
    roll = ((lambda first, n: env.rollout_uniform(SEED, first, n)) if UNI
            else (lambda first, n: env.rollout_fused(SEED, first, n)))
    env.reset()
    if not UNI:
        env.random_policy(SEED, 0)
    roll(1, burn)
    torch.cuda.synchronize()
    ck = env.checkpoint()
    acts = env.actions.clone()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run(bits):
        assert L.mrts_set_ablate(bits) == 0
        env.restore(ck)
        env.actions.copy_(acts)
        roll(burn + 1, 5)
        s.record()
        roll(burn + 6, K)
        e.record()
        e.synchronize()
        return 1e3 * s.elapsed_time(e) / K  # us per step

    ref = run(0)
    out = {}
    variants = ablate_table.selection(PHASES, os.environ.get("BITS"))  # BITS: enum names (AB_...) or bit numbers
    base, var = [], {p.bit: [] for p in variants}
    for rnd in range(5):
        for p in variants:
            base.append(run(0))
            var[p.bit].append(run(ablate_table.mask([p])))
    bmed = float(np.median(base))
    print(json.dumps({"baseline_us_per_step": bmed, "spread": [round(x, 3) for x in sorted(base)], "first": ref}), flush=True)
    for p in variants:
        m = float(np.median(var[p.bit]))
        out[p.name] = round(m - bmed, 3)
        print(json.dumps({"phase": p.name, "extra_us_per_step": round(m - bmed, 3), "runs": [round(x, 3) for x in var[p.bit]]}),
              flush=True)
    print(json.dumps({"summary": out}), flush=True)
    L.mrts_set_ablate(0)
    env.close()


if __name__ == "__main__":
    main()
