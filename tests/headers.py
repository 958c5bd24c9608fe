"""What the CPU tests read out of the C headers: the entry points include/mrts.h declares and the constants and
one-line functions of microrts_amd/csrc/mrts_internal.h.  Test infrastructure only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    """Every mrts_* function include/mrts.h declares, sorted."""
    txt = open(os.path.join(ROOT, "include", "mrts.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mrts_[a-z0-9_]+)\s*\(", txt)))


def internal_header():
    """The integer constants and one-line constexpr functions of mrts_internal.h, as Python (C's / on non-negative
    ints is //)."""
    txt = open(os.path.join(ROOT, "microrts_amd", "csrc", "mrts_internal.h")).read()
    txt = re.sub(r"//[^\n]*", "", txt)
    env = {}
    for body in re.findall(r"enum(?:\s*:\s*\w+)?\s*\{([^}]*)\}", txt):
        for k, v in re.findall(r"(\w+)\s*=\s*(\d+)\s*(?:,|$)", body):
            env[k] = int(v)
    for k, v in re.findall(r"constexpr\s+int\s+(\w+)\s*=\s*(\d+)\s*;", txt):
        env[k] = int(v)
    for name, args, expr in re.findall(r"constexpr\s+int\s+(\w+)\s*\(([^)]*)\)\s*\{\s*return\s+([^;]*);\s*\}", txt):
        params = [a.split()[-1] for a in args.split(",") if a.strip()]
        if "?" in expr:
            continue
        env[name] = eval(f"lambda {', '.join(params)}: {expr.replace('/', '//')}", env)
    return env
