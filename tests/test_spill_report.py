"""tools/spill_report.py on a hand-written ISA fragment: what counts as a spill VGPR, where the outermost loop is,
how the slots' definitions are classed; and the committed reports (profiles/spill_report_{parent,head}.md) carry
the static bar of DESIGN.md §5m for the instance the headline launches."""
import io
import os
import re

from tools import spill_report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ISA = """
_ZN12_GLOBAL__N_15k_envILi0ELi16ELi320ELb0ELb1ELb0ELb0ELb1EEEvPiPKN4mrts7KStaticENS2_4KDynE: ; @k_env
; %bb.0:
	s_load_dwordx2 s[4:5], s[0:1], 0x10
	s_mov_b32 s6, 0x2a0
	s_add_i32 s7, s2, s3
	v_writelane_b32 v9, s4, 0
	v_writelane_b32 v9, s6, 1
	v_writelane_b32 v9, s7, 2
	v_writelane_b32 v3, s7, 0               ; v3 is also used below: not a spill VGPR
	v_add_u32_e32 v3, v3, v0
	scratch_store_dword off, v1, off offset:4
.LBB0_1:                                ; the step loop
	v_readlane_b32 s8, v9, 1
	s_nop 1
	v_readlane_b32 s9, v9, 2
	v_readlane_b32 s10, v3, 5               ; a cross-lane read of the program, not a reload
	scratch_load_dword v1, off, off offset:4
.LBB0_2:
	s_cbranch_scc1 .LBB0_2
	s_cbranch_vccnz .LBB0_1
	v_readlane_b32 s4, v9, 0
	s_endpgm
	.section	.rodata
; Kernel info:
; codeLenInByte = 96
; TotalNumSgprs: 16
; NumVgprs: 10
; ScratchSize: 8
; Occupancy: 8
"""


def test_counts_and_classes():
    (sym, lines), = spill_report.kernels(ISA)
    assert spill_report.kernel_name(sym) == "k_env<0,16,320,0,1,0,0,1>"
    a = spill_report.analyse(lines)
    assert a["spill"] == ["v9"]
    assert a["stores"] == [3, 0, 0] and a["reloads"] == [0, 2, 1] and a["scratch"] == [1, 1, 0] and a["nops"] == 1
    cls = {lane: spill_report.classify(d[0]) for (_, lane), d in a["slots"].items()}
    assert cls == {0: "kernarg", 1: "immediate", 2: "other"}
    out = io.StringIO()
    assert spill_report.report(ISA, "k_env", out) == 0
    assert "| v9[1] | immediate | 0 / 1 / 0 | `s_mov_b32 s6, 0x2a0` |" in out.getvalue()


def _row(path, pat):
    for l in open(os.path.join(ROOT, "profiles", path)):
        if re.match(pat, l):
            return [c.strip() for c in l.strip().strip("|").split("|")]
    raise AssertionError(f"{path}: no row {pat}")


def test_committed_reports_hold_the_static_bar():
    parent = _row("spill_report_parent.md", r"\| `k_env<0,16,320,0,1,0,0>`")
    head = _row("spill_report_head.md", r"\| `k_env<0,16,320,0,1,0,0,1>`")
    general = _row("spill_report_head.md", r"\| `k_env<0,16,320,0,1,0,0,0>`")
    loop = lambda r, col: int(r[col].split("/")[1])  # noqa: E731
    assert general[1:] == parent[1:], "the general instance's figures changed"
    assert loop(head, 8) < loop(parent, 8), "in-loop reload sites"
    assert loop(head, 9) <= loop(parent, 9) and int(head[3]) <= 20, "scratch"
    assert int(head[2]) <= 128 and int(head[4]) == 4, "VGPRs / occupancy"
