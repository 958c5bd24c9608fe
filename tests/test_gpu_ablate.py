"""The ablation build's doubled phases leave the game as it was.

`make -C microrts_amd/csrc ablate` builds libmrts_ablate.so, in which a bit of a device flag word runs one phase of
the step a second time so that tools/ablate_price.py and tools/ablate_sq.py can price it.  A price means something
only if the second copy changes nothing: here every bit the library's own table calls AGAIN is set at once, in a child
process that loads the variant through MRTS_LIB_PATH, and everything the rollout leaves — observations, masks, action
rows, rewards, dones, the state dump of every game, the error flags — must equal what the product library leaves.
The three rollouts are the smallest that reach the kernel instances the copies sit in."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.gpu_checks import FLAG_ROLLOUTS, flag_rollout  # (the child runs gpu_checks.doubled_rollout)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABLATE = os.path.join(ROOT, "microrts_amd", "libmrts_ablate.so")


# 16x16 fused: EI_STEP16 / EI_MULTI16 in its first launches, then EI_STEADY16; 8x8 uniform without masks: EI_HELP8;
# 32x32 partially observable fused: EI_HELP32PO
@pytest.mark.parametrize("shape", list(FLAG_ROLLOUTS))
def test_doubled_phases_leave_the_game_unchanged(tmp_path, shape):
    from microrts_amd import _lib

    if not os.path.exists(ABLATE):
        pytest.skip("microrts_amd/libmrts_ablate.so is not built (make -C microrts_amd/csrc ablate)")
    if os.path.abspath(_lib.LIB_PATH) == ABLATE:
        pytest.skip("this session's own library is the variant")
    doubled, plain = str(tmp_path / "doubled.npz"), str(tmp_path / "plain.npz")
    env = dict(os.environ, MRTS_LIB_PATH=ABLATE)
    r = subprocess.run([sys.executable, "-c",
                        f"from tests.gpu_checks import doubled_rollout; doubled_rollout({doubled!r}, {shape!r})"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    flag_rollout(plain, shape)
    a, b = np.load(doubled), np.load(plain)
    assert sorted(a.files) == sorted(b.files)
    for name in a.files:
        assert np.array_equal(a[name], b[name]), name
    assert not b["flags"].any()
