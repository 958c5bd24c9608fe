"""The suite's layout rule ("Support modules"): what several files need lives in a support module, so
no file of tests/ or tools/ imports from a test module, the GPU guard exists once (tests/gpu_support.py) and no
test file grows its own copy of it or of the pointer helper.  A test module that is somebody's library cannot be
moved or renamed, and its helpers' meaning hides behind underscore names.  CPU only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every way of reaching a test module: the dotted module name after `from` or `import`, or the bare module name after
# `from tests import` (alone or in a list), also inside the string a child process gets through `python -c`
TEST_IMPORT = re.compile(r"\btests\.test_\w+|\bfrom\s+tests\s+import\s+(?:\(\s*)?(?:\w+\s*(?:as\s+\w+\s*)?,\s*)*test_\w+")
GUARD = "torch.cuda." + "is_available"
OWN_HELPER = re.compile(r"^\s*def\s+(_torch|_p)\s*\(", re.M)
# files the scan must have read, or it looked in the wrong place (an empty scan cannot pass)
MUST_SEE = {"tests/test_gpu_parity.py", "tests/test_kats.py", "tests/gpu_support.py", "tests/golden/rollouts.py",
            "tools/soak_long.py"}


def _sources():
    """relative path -> text of every Python file under tests/ and tools/ (this file's own patterns do not count)"""
    out = {}
    for top in ("tests", "tools"):
        for d, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if x != "__pycache__"]
            for fn in files:
                path = os.path.join(d, fn)
                if fn.endswith(".py") and os.path.abspath(path) != os.path.abspath(__file__):
                    with open(path, errors="replace") as f:
                        out[os.path.relpath(path, ROOT).replace(os.sep, "/")] = f.read()
    return out


def _hits(pattern, text):
    return [f"line {text.count(chr(10), 0, m.start()) + 1}: {m.group(0)}" for m in pattern.finditer(text)]


def test_the_patterns_match_what_they_forbid():
    pkg, mod = "tests", "test_kats"  # (in pieces: the lines below must not match the patterns themselves)
    for line in (f"from {pkg}.{mod} import HP", f"import {pkg}.{mod}", f"from {pkg} import {mod} as T",
                 f"from {pkg} import oracle_py, {mod}", f'[sys.executable, "-c", "from {pkg}.{mod} import f; f()"]'):
        assert TEST_IMPORT.search(line), line
    for line in ("from tests import oracle_py", "from tests.defs import SEED", "tests/test_kats.py", "pytest tests -k test_kats"):
        assert not TEST_IMPORT.search(line), line
    assert OWN_HELPER.search("def _torch():") and OWN_HELPER.search("    def _p(t):") and not OWN_HELPER.search("def _parse(d):")


def test_no_file_imports_from_a_test_module():
    src = _sources()
    assert MUST_SEE <= set(src), f"the scan missed {sorted(MUST_SEE - set(src))}"
    bad = {p: _hits(TEST_IMPORT, t) for p, t in src.items() if TEST_IMPORT.search(t)}
    assert not bad, f"imports from test modules (move what is shared into a support module): {bad}"


def test_one_gpu_guard_and_no_private_copies():
    src = {p: t for p, t in _sources().items() if p.startswith("tests/")}
    missed = {p for p in MUST_SEE if p.startswith("tests/")} - set(src)
    assert not missed, f"the scan missed {sorted(missed)}"
    assert GUARD in src["tests/gpu_support.py"], "tests/gpu_support.py no longer holds the GPU guard"
    elsewhere = sorted(p for p, t in src.items() if GUARD in t and p != "tests/gpu_support.py")
    assert not elsewhere, f"{GUARD} outside tests/gpu_support.py (use torch_gpu()): {elsewhere}"
    own = {p: _hits(OWN_HELPER, t) for p, t in src.items() if OWN_HELPER.search(t)}
    assert not own, f"private copies of the GPU guard / the pointer helper (use gpu_support.torch_gpu / ptr): {own}"
