#!/usr/bin/env python3
"""SGPR-spill and scratch traffic of the k_env instances, read off the device ISA (no GPU needed).

The register allocator spills SGPRs into the lanes of VGPRs it sets aside: a spill store is
`v_writelane_b32 vS, sN, <lane>`, a reload `v_readlane_b32 sN, vS, <lane>` — each a VALU instruction in kernels
that are VALU-issue bound, each reload in front of a scalar use.  VGPR spills go to scratch memory
(`scratch_store_*` / `scratch_load_*`).  Per instance this prints the register counts, ScratchSize and occupancy,
the spill stores / reload sites / scratch sites before, inside and after the outermost loop (the multi-step
kernels' step loop), the `s_nop` count, and for every spill slot (spill VGPR, lane) the instruction that defined
the value stored there, classed as

  immediate  every source operand is a literal (a constant the allocator chose to keep in a register),
  kernarg    a scalar memory load (a kernel-argument field or something addressed by one),
  other      anything else (computed values: per-game bases, lane masks, ...).

It counts lane reads / writes, scratch operations and s_nop, nothing else.  A VGPR counts as a spill VGPR when
lane writes from SGPRs at constant lanes and lane reads at constant lanes are its only uses.

Usage: python tools/spill_report.py FILE.s [--detail REGEX]     read an existing ISA file
       python tools/spill_report.py --build DIR [--detail REGEX] run `make isa ISA_OUT=DIR/mrts_kernels.s` first
--detail: instances (by their printed name) whose slots are listed; default: the 16x16 multi-step instances.
"""
import argparse
import os
import re
import subprocess
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANE_W = re.compile(r"^v_writelane_b32 (v\d+), (s\d+|vcc_lo|vcc_hi|exec_lo|exec_hi|ttmp\d+|m0), (\d+)$")
LANE_R = re.compile(r"^v_readlane_b32 (s\d+|vcc_lo|vcc_hi|exec_lo|exec_hi|ttmp\d+|m0), (v\d+), (\d+)$")
BRANCH = re.compile(r"^s_c?branch\w*\s+(\.LBB\w+)$")
LABEL = re.compile(r"^(\.LBB\w+):")
VREG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")
READS_MORE = ("s_cselect", "s_cmov", "s_addc", "s_subb", "s_bitset", "s_getreg", "s_getpc", "s_memtime", "s_memrealtime")
NO_SDST = ("s_cmp", "s_bitcmp", "s_waitcnt", "s_nop", "s_setprio", "s_setreg", "s_barrier", "s_sleep", "s_cbranch", "s_branch",
           "s_endpgm", "s_sendmsg", "s_set", "s_clause", "s_delay", "s_inst_prefetch", "s_code_end")
LITERAL = re.compile(r"^(-?\d+|0x[0-9a-fA-F]+|-?\d*\.\d+(e[-+]?\d+)?|[\w.$]+@\w+(@\w+)?)$")


def kernel_name(sym):
    """k_env's template arguments out of its mangled name: k_env<0,16,320,0,1,0,0,1>."""
    m = re.search(r"k_envI((?:L[ib]\d+E)+)E", sym)
    if not m:
        return sym
    return "k_env<" + ",".join(re.findall(r"L[ib](\d+)E", m.group(1))) + ">"


def kernels(text):
    """(symbol, instruction lines, metadata) of every k_env instance in an ISA file."""
    out, cur, sym = [], None, None
    for line in text.split("\n"):
        m = re.match(r"^(_Z\w*k_env\w*):", line)
        if m:
            sym, cur = m.group(1), []
            continue
        if cur is None:
            continue
        cur.append(line)
        if line.startswith("; Occupancy:"):
            out.append((sym, cur))
            cur = None
    return out


def meta(lines, key):
    for l in lines:
        m = re.match(r"^; %s:? (?:= )?(\d+)" % re.escape(key), l)
        if m:
            return int(m.group(1))
    return None


def sregs(op):
    """The scalar registers an operand names."""
    m = re.match(r"^s\[(\d+):(\d+)\]$", op)
    if m:
        return {"s%d" % i for i in range(int(m.group(1)), int(m.group(2)) + 1)}
    if op in ("vcc", "exec"):
        return {op + "_lo", op + "_hi"}
    return {op} if re.match(r"^(s\d+|vcc_lo|vcc_hi|exec_lo|exec_hi|m0|ttmp\d+)$", op) else set()


def classify(ins):
    if ins is None:
        return "other"
    mnem, _, rest = ins.partition(" ")
    if mnem.startswith(("s_load_", "s_buffer_load_")):
        return "kernarg"
    ops = [o.strip() for o in rest.split(",")]
    srcs = ops[1:]
    # (not the instructions that also read SCC or their own destination)
    if mnem.startswith(READS_MORE):
        return "other"
    if mnem.startswith("s_") and srcs and all(LITERAL.match(o) for o in srcs):
        return "immediate"
    return "other"


def analyse(lines):
    ins = []  # (text, label or None)
    for l in lines:
        t = l.split(";")[0].strip()
        if not t or t.startswith((".", "//")) and not LABEL.match(t):
            continue
        ins.append(t)
    # spill VGPRs: only ever used by constant-lane writes from scalar registers and constant-lane reads
    cand, other = set(), set()
    for t in ins:
        w, r = LANE_W.match(t), LANE_R.match(t)
        if w:
            cand.add(w.group(1))
        elif r:
            pass
        else:
            if t.startswith(("scratch_", "s_waitcnt")) or LABEL.match(t):
                continue
            for m in VREG.finditer(t):
                if m.group(1) is not None:
                    other.add("v" + m.group(1))
                else:
                    other.update("v%d" % i for i in range(int(m.group(2)), int(m.group(3)) + 1))
    spill = cand - other
    # the outermost loop: the widest backward branch, grown by every loop that overlaps it
    pos = {LABEL.match(t).group(1): i for i, t in enumerate(ins) if LABEL.match(t)}
    loops = []
    for i, t in enumerate(ins):
        b = BRANCH.match(t)
        if b and b.group(1) in pos and pos[b.group(1)] <= i:
            loops.append((pos[b.group(1)], i))
    lo = hi = -1
    if loops:
        lo, hi = max(loops, key=lambda p: p[1] - p[0])
        grown = True
        while grown:
            grown = False
            for a, b in loops:
                if a <= hi and b >= lo and (a < lo or b > hi):
                    lo, hi, grown = min(lo, a), max(hi, b), True
    where = lambda i: 0 if i < lo else (1 if i <= hi else 2)
    stores, reloads, scratch = [0, 0, 0], [0, 0, 0], [0, 0, 0]
    slots = {}  # (vgpr, lane) -> [defining instruction of each store]
    reads = Counter()
    lastdef = {}
    nops = 0
    for i, t in enumerate(ins):
        if LABEL.match(t):
            continue
        w, r = LANE_W.match(t), LANE_R.match(t)
        if w and w.group(1) in spill:
            stores[where(i)] += 1
            slots.setdefault((w.group(1), int(w.group(3))), []).append(lastdef.get(w.group(2)))
            continue
        if r and r.group(2) in spill:
            reloads[where(i)] += 1
            reads[(r.group(2), int(r.group(3)), where(i))] += 1
            lastdef[r.group(1)] = t
            continue
        if t.startswith("scratch_"):
            scratch[where(i)] += 1
        if t.startswith("s_nop"):
            nops += 1
        mnem, _, rest = t.partition(" ")
        if mnem.startswith(("s_", "v_readlane", "v_readfirstlane", "v_cmp", "v_cmpx")) and rest and not mnem.startswith(NO_SDST):
            ops = [o.strip() for o in rest.split(",")]
            for reg in sregs(ops[0]):
                lastdef[reg] = t
            if mnem.startswith(("v_cmpx", "s_and_saveexec", "s_or_saveexec", "s_andn2_saveexec", "s_xor_saveexec")):
                lastdef["exec_lo"] = lastdef["exec_hi"] = t
    return dict(spill=sorted(spill, key=lambda v: int(v[1:])), loop=(lo, hi), n=len(ins), stores=stores, reloads=reloads,
                scratch=scratch, nops=nops, slots=slots, reads=reads)


def report(text, detail, out=sys.stdout):
    p = lambda *a: print(*a, file=out)
    ks = kernels(text)
    if not ks:
        p("no k_env instance in the ISA")
        return 1
    p("| instance | SGPRs | VGPRs | ScratchSize | occupancy | code bytes | spill VGPRs | spill stores pre/loop/post | "
      "reload sites pre/loop/post | scratch sites pre/loop/post | s_nop |")
    p("|---|---|---|---|---|---|---|---|---|---|---|")
    res = []
    for sym, lines in ks:
        a = analyse(lines)
        name = kernel_name(sym)
        res.append((name, a))
        tri = lambda v: "%d / %d / %d" % tuple(v)
        p(f"| `{name}` | {meta(lines, 'TotalNumSgprs')} | {meta(lines, 'NumVgprs')} | {meta(lines, 'ScratchSize')} | "
          f"{meta(lines, 'Occupancy')} | {meta(lines, 'codeLenInByte')} | {' '.join(a['spill']) or '-'} | {tri(a['stores'])} | "
          f"{tri(a['reloads'])} | {tri(a['scratch'])} | {a['nops']} |")
    for name, a in res:
        if not re.search(detail, name):
            continue
        p(f"\n### `{name}`: spill slots ({len(a['slots'])}), outermost loop = instructions {a['loop'][0]}..{a['loop'][1]} of {a['n']}\n")
        kinds = Counter()
        p("| slot | class | reloads pre/loop/post | defined by |")
        p("|---|---|---|---|")
        for (v, lane), defs in sorted(a["slots"].items(), key=lambda kv: (int(kv[0][0][1:]), kv[0][1])):
            cls = sorted({classify(d) for d in defs})
            c = cls[0] if len(cls) == 1 else "other"
            kinds[c] += 1
            rd = [a["reads"][(v, lane, w)] for w in range(3)]
            shown = "; ".join(dict.fromkeys(d or "(live-in)" for d in defs))
            p(f"| {v}[{lane}] | {c} | {rd[0]} / {rd[1]} / {rd[2]} | `{shown}` |")
        p(f"\nslots by class: immediate {kinds['immediate']}, kernarg {kinds['kernarg']}, other {kinds['other']}")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("isa", nargs="?", help="an ISA file (hipcc --cuda-device-only -S)")
    ap.add_argument("--build", metavar="DIR", help="run the Makefile's isa recipe into DIR/mrts_kernels.s and read that")
    ap.add_argument("--detail", default=r"^k_env<0,16,320,0,1,", help="regex of the instances whose slots are listed")
    a = ap.parse_args()
    if bool(a.isa) == bool(a.build):
        ap.error("give an ISA file or --build DIR")
    path = a.isa
    if a.build:
        os.makedirs(a.build, exist_ok=True)
        path = os.path.join(os.path.abspath(a.build), "mrts_kernels.s")
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "microrts_amd", "csrc"), "isa", "ISA_OUT=" + path])
    sys.exit(report(open(path).read(), a.detail))


if __name__ == "__main__":
    main()
