#!/usr/bin/env python3
"""Index of the reference's Java sources for tests/test_citations.py: for every `*.java` file its path in
the reference tree, its number of lines and, per method name, the line spans of the definitions found in it.
Names and line numbers only — no program text — so the citation checks run from the checkout alone.

Output: tests/golden/java_index.json  {"<path in the reference tree>": [lines, {"<method>": [[first, last], ...]}]}

Run once where the reference snapshot is unpacked:
    python tests/golden/make_java_index.py <reference root>
"""
import collections
import glob
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DEF = re.compile(r"^\s*(?:public|private|protected|static|final|synchronized|abstract|\s)*[\w<>\[\],\s]+?\s(\w+)\s*\([^;]*$")


def methods(path):
    """-> ({method name: [(first line, last line), ...]}, number of lines): a definition line and its body up to
    the brace that closes it (or the `;` of an abstract declaration)."""
    lines = open(path, errors="replace").read().split("\n")
    out = collections.defaultdict(list)
    for i, line in enumerate(lines):
        m = DEF.match(line)
        if not m or m.group(1) in ("if", "for", "while", "switch", "catch", "return", "new"):
            continue
        depth, started, j = 0, False, i
        while j < len(lines):
            for ch in lines[j]:
                depth += (ch == "{") - (ch == "}")
                started = started or ch == "{"
            if (started and depth <= 0) or (not started and lines[j].rstrip().endswith(";")):
                break
            j += 1
        out[m.group(1)].append((i + 1, j + 1))
    return out, len(lines) - (lines[-1] == "")


def main():
    ref = os.path.abspath(sys.argv[1])
    index = {}
    for p in sorted(glob.glob(os.path.join(ref, "**", "*.java"), recursive=True)):
        defs, n = methods(p)
        index[os.path.relpath(p, ref)] = [n, defs]
    dst = os.path.join(HERE, "java_index.json")
    json.dump(index, open(dst, "w"), separators=(",", ":"), sort_keys=True)
    print(f"{dst}: {len(index)} files, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
