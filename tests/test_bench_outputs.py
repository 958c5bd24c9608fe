"""bench.py's plain run and --dump-outputs: the line of a plain run carries the headline figures and none of
--full's blocks, --steps sets the number of timed steps, and the dumped arrays are what the timed path's last
step left in the caller's tensors — compared exactly with the same call sequence made here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_dumps_the_last_timed_step(tmp_path):
    import torch

    from microrts_amd import DeviceVecEnv

    G, B, W, K = 32, 30, 2, 4  # games, burn-in, warmup, timed steps: one small c3-shaped run
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs", str(G), "--burnin", str(B),
                        "--warmup", str(W), "--steps", str(K), "--dump-outputs", str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == K and line["warmup"] == W and line["unit"] == "env-steps/s" and line["higher_is_better"] is True
    assert line["dtype"] == "int32" and line["metric"] == bench.METRIC
    assert line["ms_per_step"] > 0 and abs(line["value"] - G / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    for block in ("roofline", "cpu_baseline", "full_contract", "with_gather", "other_policy_form", "single_step_launches",
                  "configs"):
        assert block not in line, block
    # the same calls as the timed path (bench.main: fused policy, native rollout launches of B, W and K steps)
    env = DeviceVecEnv(2 * G, 0, 2000, [os.path.join(ROOT, bench.MAP)] * (2 * G), seed=bench.SEED)
    env.reset()
    env.random_policy(bench.SEED, 0)
    for first, n in ((0, B), (B, W), (B + W, K)):
        env.rollout_fused(bench.SEED, first + 1, n)
    torch.cuda.synchronize()
    want = {"obs": env.obs, "masks": env.masks, "actions": env.actions, "reward": env.reward, "done": env.done}
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in want)
    total = 0
    for k, t in want.items():
        got = np.load(out / (k + ".npy"))
        total += got.nbytes
        assert got.dtype == (np.float64 if k == "reward" else np.float32), k
        assert got.shape == tuple(t.shape) and np.array_equal(got, t.cpu().numpy()), k
    assert total <= 64 << 20
    assert np.count_nonzero(np.load(out / "obs.npy")) and np.count_nonzero(np.load(out / "masks.npy"))
    env.close()
