"""Every build switch of microrts_amd/csrc is built by something committed: a name that a
preprocessor conditional tests, or that an `#ifndef X / #define X` default introduces, appears in the Makefile or in
a file under tools/ or tests/.  A switch added to A/B one experiment is folded into the code it selected once the
result is in; left behind, nothing compiles its other value and every later change has to read past it.  CPU only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "microrts_amd", "csrc")
NAME = re.compile(r"MRTS_[A-Z0-9_]+")  # (no \b: the Makefile says -DMRTS_X)
# the switches in use: the six diagnostic builds, and the two a test / a tool builds at the other value
KEPT = {"MRTS_PHASE_TIMING", "MRTS_SPAN_ONLY", "MRTS_MILES_STEP", "MRTS_NO_MILESTONES", "MRTS_ABLATE", "MRTS_LANE_AUDIT",
        "MRTS_ISSUE_BOTH", "MRTS_NO_PO_HELPER"}
# switches nothing builds that are still there, each with the reason it could not be folded; a name leaves this list
# with its switch (the test fails on an entry the scan no longer finds)
UNFOLDED = {
    "MRTS_PO_VRES": "rejected in round 6; folding its dead arm changes the device code of the `timing` and `ablate` "
                    "builds (the default library's stays byte-identical), and the fold of the others rested on identity",
}


def _read(path):
    with open(path, errors="replace") as f:
        return f.read()


def _switches():
    """name -> "file:line" of its first test in csrc/*"""
    found = {}
    for fn in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, fn)
        if fn == "Makefile" or not os.path.isfile(path):
            continue
        for no, line in enumerate(_read(path).splitlines(), 1):
            m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b(.*)", line)
            if m:
                for name in NAME.findall(m.group(2).split("//")[0]):
                    found.setdefault(name, f"{fn}:{no}")
    public = set(NAME.findall(_read(os.path.join(ROOT, "include", "mrts.h"))))
    return {n: at for n, at in found.items() if n not in public}


def _users():
    """the text that may build a switch: the Makefile, tools/ and tests/ (this file's own list does not count)"""
    texts = [_read(os.path.join(CSRC, "Makefile"))]
    for top in ("tools", "tests"):
        for d, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [x for x in dirs if x not in ("golden", "__pycache__")]
            for fn in files:
                path = os.path.join(d, fn)
                if os.path.abspath(path) != os.path.abspath(__file__) and os.path.getsize(path) < (1 << 20) \
                        and not fn.endswith((".pyc", ".so", ".npy", ".npz", ".gz")):
                    texts.append(_read(path))
    return set(NAME.findall("\n".join(texts)))


def test_every_build_switch_is_built_by_something_committed():
    sw = _switches()
    assert KEPT <= set(sw), f"the scan missed {sorted(KEPT - set(sw))}"  # (an empty scan cannot pass)
    used = _users()
    assert set(UNFOLDED) <= set(sw), f"no longer in the source, drop from UNFOLDED: {sorted(set(UNFOLDED) - set(sw))}"
    assert not set(UNFOLDED) & used, f"built by something now, drop from UNFOLDED: {sorted(set(UNFOLDED) & used)}"
    orphans = {n: at for n, at in sw.items() if n not in used and n not in UNFOLDED}
    assert not orphans, (f"build switches that no Makefile target, tool or test builds: {orphans} — fold each into the "
                         f"code its default selects (DESIGN.md §9)")
