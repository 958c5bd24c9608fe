"""Every game of the benchmark configurations against the CPU oracle (VERDICT r4 "next" #2).

test_headline_parity.py replays a 65-game sample of each bench shape; round 4's hand-run soak
(now tools/soak_full_parity.py) compared every game and found a bit-exactness bug the sample had missed.
These tests are that soak in the driver's `-m gpu` suite: the shipped benchmark form of c3 (4096 self-play
games on basesWorkers16x16, fused masked policy, delta masks), c5 (2048 partially observable games on
BWDistantResources32x32, max_units 256, the render helper wave) and c2 (1024 games on basesWorkers8x8,
unmasked uniform rows drawn by the step kernel), each run as ONE native rollout call per point — a
1000-step burn-in, then a K = 20 and a K = 200 multi-step launch — and at every point every slot's
observation, reward, done, mask buffer (c3 / c5), the action rows the launch left in the tensor and the
canonical state dump (units in list order, assignments in LinkedHashMap order) must equal the oracle's
(tests.gpu_checks.every_game, which tools/soak_long.py runs over longer horizons).

The oracle side is one OracleVecClient per shard of games, each on its own Python thread, stepping in
native code (oref_rollout_policy: getMasks, then the same Philox rows the GPU draws, then gameStep —
JNIGridnetVecClient.java:213-316), so no GPU-produced action ever enters the oracle.  UTT v1 +
CANCEL_BOTH draws no Java random numbers, so each oracle game is an exact replica of its GPU game.
"""
import pytest

from tests.gpu_checks import every_game

pytestmark = pytest.mark.gpu


def test_every_game_c3():
    """BASELINE configs[2] as bench.py times it, all 4096 games (8192 slots)."""
    every_game("c3")


def test_every_game_c5():
    """BASELINE configs[4] per GPU, all 2048 partially observable games, with the render helper wave
    (round 4's soak found its stale-value case here)."""
    every_game("c5")


def test_every_game_c2():
    """BASELINE configs[1] as bench.py times it, all 1024 games, unmasked uniform rows."""
    every_game("c2")
