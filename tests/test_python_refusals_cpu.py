"""The Python package's refusals are the parent's, word for word: every case of tests/python_refusal_cases.py raises
the exception type and the full text recorded in tests/golden/python_refusals_parent.json (recorded from the commit
before the package got its one packed-row check; see that module).  CPU only, no library."""
import json
import os

import pytest

from tests import python_refusal_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "python_refusals_parent.json")))
CASES = [(name, call) for group in C.cases().values() for name, _, call in group]


def test_every_case_is_in_the_golden_and_nothing_else():
    names = [name for name, _ in CASES]
    assert len(set(names)) == len(names) >= 90
    assert sorted(names) == sorted(GOLDEN)
    # both wordings of each refusal that the two packed families word differently are among them
    texts = {t for _, t in GOLDEN.values()}
    assert {"logits: rows * H*W must be below 2^31", "packed: rows * H*W must be below 2^31",
            "index: rows * H*W must be below 2^31", "packed: 3 rows for 4 rows of logits (pass an index to gather)",
            "index: expected an int32 tensor [rows]", "index: expected a torch tensor, got list",
            "out: 42 words is not 1 + cap * 5 for a cap in [1, H*W = 16]",
            "out: 40 words is not 23 + 2 * cap for a cap in [1, H*W = 16]"} <= texts


@pytest.mark.parametrize("name,call", CASES, ids=[name for name, _ in CASES])
def test_refusal_is_the_parents(name, call):
    assert C.answer(call) == GOLDEN[name]
