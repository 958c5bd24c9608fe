#!/usr/bin/env python3
"""What an agent-vs-bot step costs per opponent: 4096 games of basesWorkers16x16, the masked random policy as the
agent, against PassiveAI, RandomBiasedAI and the native LightRush (not bench.py: nothing reads this but people).

Per opponent: a warm-up, then chunks of steps between two device events until at least --seconds of device time
are timed (policy kernel + step kernel per step, as a learner's loop issues them).  One JSON line: env-steps/s and
microseconds per step of every opponent.

    python tools/bench_opponents.py [--opponents PassiveAI RandomBiasedAI LightRush] [--games 4096] [--seconds 2]
    MRTS_LIB_PATH=<another build of libmrts.so> python tools/bench_opponents.py --opponents PassiveAI RandomBiasedAI
    MRTS_LIB_PATH=microrts_amd/libmrts_timing.so python tools/bench_opponents.py --phases   # make -C microrts_amd/csrc timing

--phases (the timing build's per-phase shader clocks): mean cycles per game step of every phase slot, the LightRush
slots named — where getAction spends its time.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x5EEDC0DE
NPH = 32
PHASE_NAMES = {0: "load", 2: "agent decode", 3: "agent issue", 4: "cycle (+ issue without LightRush)", 5: "outcome + reset",
               6: "observation", 7: "compaction", 8: "masks (stash)", 9: "masks + policy rows", 10: "store",
               25: "LightRush behaviours + scans", 26: "LightRush A*", 27: "LightRush translateActions (rest)",
               28: "LightRush issue"}


def run(opponent, a, lib):
    import torch

    from microrts_amd import DeviceVecEnv

    env = DeviceVecEnv(0, a.games, 2000, [os.path.join(ROOT, a.map)] * a.games, ai2s=[opponent] * a.games, seed=1)
    env.reset()
    step = 0
    for _ in range(a.warmup):
        env.random_policy(SEED, step)
        env.step()
        step += 1
    env.synchronize()
    if a.phases:
        buf = (ctypes.c_ulonglong * (2 * NPH))()
        lib.mrts_phase_times(buf, 1)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms, n = 0.0, 0
    while ms < 1e3 * a.seconds:
        s.record()
        for _ in range(a.chunk):
            env.random_policy(SEED, step)
            env.step()
            step += 1
        e.record()
        e.synchronize()
        ms += s.elapsed_time(e)
        n += a.chunk
    out = {"env_steps_per_s": round(a.games * n / (1e-3 * ms), 1), "us_per_step": round(1e3 * ms / n, 2), "steps": n}
    if a.phases:
        lib.mrts_phase_times(buf, 1)
        out["cycles_per_game_step"] = {PHASE_NAMES.get(i, f"p{i}"): round(buf[i] / (n * a.games), 1)
                                       for i in range(NPH) if buf[i]}
    assert not env.error_flags().any()
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--opponents", nargs="+", default=["PassiveAI", "RandomBiasedAI", "LightRush"])
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--map", default="maps/16x16/basesWorkers16x16.xml")
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--chunk", type=int, default=100, help="steps between two device events")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed device time per opponent, at least")
    ap.add_argument("--phases", action="store_true", help="per-phase cycles (needs the timing build in MRTS_LIB_PATH)")
    ap.add_argument("--label", default=None, help="copied into the result line (which build this is)")
    a = ap.parse_args()
    from microrts_amd import _lib

    lib = _lib.load()
    if a.phases:
        if not hasattr(lib, "mrts_phase_times"):
            sys.exit("--phases needs the timing build: MRTS_LIB_PATH=microrts_amd/libmrts_timing.so")
        lib.mrts_phase_times.argtypes = [ctypes.c_void_p, ctypes.c_int]
    res = {o: run(o, a, lib) for o in a.opponents}
    print(json.dumps({"tool": "bench_opponents", "label": a.label, "library": os.path.relpath(_lib.LIB_PATH, ROOT),
                      "games": a.games, "map": a.map, "agent": "masked random policy", "warmup_steps": a.warmup,
                      "opponents": res}), flush=True)


if __name__ == "__main__":
    main()
