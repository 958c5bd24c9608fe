"""What the library answers to calls it refuses — the return code and mrts_last_error() — is what it answered
before every entry point went through the one entry guard (mrts_host.cpp guarded / guardedCall): the table of
tests/refusal_cases.py against tests/golden/refusals_parent.json, recorded by that module from the parent commit's
library.  After the refusals the same handle resets and steps like the oracle: no refusal touched its bookkeeping."""
import json
import os

import numpy as np
import pytest

from tests.gpu_support import torch_gpu
from tests import oracle_py, refusal_cases

GOLDEN = os.path.join(refusal_cases.ROOT, "tests", "golden", "refusals_parent.json")


@pytest.mark.gpu
def test_gpu_refusals_are_the_parents():
    torch = torch_gpu()
    want = json.load(open(GOLDEN))
    L, lib_mod, env, fm = refusal_cases.handles()
    got = refusal_cases.answers(L, lib_mod, env, fm)
    assert len(want) >= 100 and [n for n, _, _ in got] == [n for n, _, _ in want], "the table and its record list the same cases"
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, f"{len(wrong)} refusals differ from the parent's (got, want): {wrong[:5]}"
    assert {rc for _, rc, _ in got} >= {-22, -28, -95, -2}, "EINVAL, ENOSPC, ENOTSUP and ENOENT all occur"
    # the handle is as it was: a reset and a masked step equal the oracle's
    S = 3
    ref = oracle_py.OracleVecClient(2, 1, 2000, [refusal_cases.M8] * S, bot_kinds=[oracle_py.BOT_PASSIVE], seed=11)
    env.reset()
    o, r, d = ref.reset()
    env.synchronize()
    m = ref.get_masks(0)
    assert np.array_equal(env.obs.cpu().numpy(), o) and np.array_equal(env.masks.cpu().numpy(), m)
    acts = np.stack([oracle_py.policy(m[s], 77, s, 0, 0) for s in range(S)])
    env.actions.copy_(torch.as_tensor(acts))
    env.step()
    o, r, d = ref.step(acts)
    env.synchronize()
    assert np.array_equal(env.obs.cpu().numpy(), o) and np.array_equal(env.reward.cpu().numpy(), r)
    assert np.array_equal(env.done.cpu().numpy(), d) and np.array_equal(env.masks.cpu().numpy(), ref.get_masks(0))
    assert not env._h.error_flags().any()
    env.close()
    fm.close()
    ref.close()
