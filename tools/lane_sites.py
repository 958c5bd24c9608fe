#!/usr/bin/env python3
"""The cross-lane read sites of the kernels (microrts_amd/csrc: the three .hip units and mrts_device.h) and why each
reads only lanes that are active.

Lists every `rl()` (readlane) call and every DPP reduction / prefix-sum call site by enclosing function, with the
argument that its source lanes executed the definition it reads: the call itself runs in wave-uniform control flow
(every lane of the game's wave active — so even if the compiler sinks the source's definition next to the use, it
is computed there for every lane), and the lanes it reads hold a value defined for them.  A site in a function
without an entry below makes the script fail, so the table cannot silently fall behind the code.  The run-time
counterpart is the audit build (`make -C microrts_amd/csrc audit`, tests/test_zz_lane_audit.py).

Usage: python tools/lane_sites.py [--markdown]
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "microrts_amd", "csrc")
# the audit build's unit ids (MRTS_UNIT) in order, then the header they share
UNITS = ["mrts_kernels.hip", "mrts_policy.hip", "mrts_aux.hip"]
SRCS = UNITS + ["mrts_device.h"]

# function -> why its cross-lane reads are safe
WHY = {
    "wave_reduce": "helper: DPP over all 64 lanes then lane 63 — every caller below is in uniform flow; the source "
                   "value is a select defined on every lane",
    "wave_incl_sum": "helper: DPP prefix sum — callers in uniform flow with the operand defined on every lane",
    "wave_min": "wrapper of wave_reduce", "wave_sum": "wrapper of wave_reduce",
    "loadHeader": "called from load() / nextStep() in uniform flow; hv = `l < H_WORDS ? s[l] : 0` is a select on "
                  "every lane, and the lanes read (H_TIME..H_SEQ < H_WORDS) loaded their word",
    "load": "H_FWD read in uniform flow from the same header register as loadHeader",
    "auditIndex": "audit build only (carryIndex's cross-check, called in uniform flow at the step's start): the "
                  "reductions take selects defined on every lane (0 / 1 outside the PRODUCE lanes)",
    "baseReservations": "wave_sum of per-lane sums accumulated in a uniform `for (o0 ...)` loop (every lane adds 0 "
                        "outside the list)",
    "cellRank": "uniform loop over the candidate mask m (a ballot); c is the caller's per-lane cell, defined on every "
                "lane (decode / issue paths compute it before the candidate test)",
    "prodCosts": "called in uniform flow; cost | player << 16 is computed on every lane before the uniform loop over "
                 "ballot(np), which reads only np lanes; the reductions take every lane's value (0 / 1 outside np)",
    "issueBothWrite": "called in uniform flow (the merged test is wave-uniform); key is derived from the lane's unit "
                      "word on every lane before the uniform loop over ballot(cand), which reads only cand lanes "
                      "(l < nu: a loaded unit word)",
    "acceptChainReg": "tpos / cost / keyR / bv are defined on every lane before the uniform loops over ballots or "
                      "r < n; the readlanes sit outside the lane tests (round 5 moved the collision scan's read out "
                      "of `if (up && ...)`); bv's conditional update is on its own lane",
    "acceptChain": "general path (> 64 reservation words): k = ctz(ballot(rank == r)) in a uniform r loop; usesPos, "
                   "tpos, cost defined on every lane",
    "issueOne": "wave_min over every lane's candidate in a uniform loop",
    "buildIndex": "key (-1 or cost | player) is set for every lane in the uniform `for (o0 ...)` body before the "
                  "ballot; the walk reads only lanes of that ballot",
    "issueBatch": "uniform loops over ballots of act / mp / np lanes; s, rank, t, prm, tx, ty, ut are the caller's "
                  "per-lane values for act lanes; ntgt / pl / ncost are written inside `if (mp)` and read only from "
                  "mp (or np ⊂ mp) lanes, after the branch reconverges; the checkDup readlanes were moved out of the "
                  "lane test in round 5",
    "pickRandomBiased": "every value is wave-uniform (uniu / uni); the `idx - seen < cnt` branch is uniform; qc is "
                        "set on every lane of the uniform q0 loop (0 outside the list) before the ballot",
    "snapshot": "observer words ow defined on every lane of the uniform q0 loop; k1 / k2 come from ballot(obs)",
    "cycle": "R <= 64 branch and the loops are uniform; myseq is a select on every lane; cu / a / prm are written "
             "for lanes k < R and read only from lanes of work ⊂ {k < R}",
    "cycleLanes": "sq / cu / a / prm written for lanes l < nu under `if (l < nu)`; read only from lanes of "
                  "work = ballot(wk) ⊂ {l < nu}, in a uniform loop",
    "ablCycleRank": "ablation build only, cycleLanes' ready test and rank once more: called from its top level under a "
                    "wave-uniform test of the ablation word; q2 is a laundered copy of sq on every lane, read from lanes "
                    "of a ballot ⊂ {l < nu}",
    "ablExecLoop": "ablation build only, cycleLanes' execute loop without the executes: the same uniform loop over "
                   "work = ballot(wk), reading cu / a / prm from its lanes",
    "ablMaskBitsDir": "ablation build only, writeMasksSteady's quad bits once more: quadOr of u0..u2, each set on every "
                      "lane, in the uniform pass loop under a wave-uniform test of the ablation word",
    "quadOr": "helper: DPP quad_perm OR within each quad — called by maskBitsQuads / writeMasksSteady in uniform flow (outside their lane "
              "tests) with v defined on every lane (0 for lanes without a unit)",
    "maskBitsQuads": "quadOr of v0..v2, each set on every lane (0 unless the lane's quad has a unit) before the calls, in "
                     "the uniform pass loop",
    "closerMin": "wave_min of per-lane minima of a uniform `for (o ...)` loop",
    "farAttackBits": "`if (!ballot(far)) return` is uniform; the loop over the owned mask is uniform; cuLane is the "
                     "caller's unit word of every lane < nu (owned ⊂ {l < nu})",
    "writeMasksUnits": "wave_incl_sum / lane-63 read of a count defined on every lane (0 beyond the row-set words)",
    "writeMasksLanes": "as writeMasksUnits: n = popc(gone) on every lane, uniform flow",
    "rowInclSum": "helper: wave_incl_sum's four row_shr steps (a prefix sum inside each 16-lane row) — called by "
                  "writeMasksSteady in uniform flow with the operand defined on every lane",
    "writeMasksSteady": "steady instance: n = popc(gone) is set on every lane (0 beyond the 16 row-set words) before "
                        "rowInclSum, and lane 15, read for the total, is a lane of the wave; quadOr of v0..v2, each "
                        "set on every lane (0 unless the lane's quad has a unit) in the uniform pass loop; the "
                        "ablation copies sit under wave-uniform tests of the ablation word",
    "balancePerm": "the last wave of an XCD class sorts in uniform flow (`if (ballot(!ok)) return` is uniform); "
                   "sum is each lane's 4-bin total",
    "k_policy_delta": "kernel level, before any divergence: every lane's popc(dirty)",
    "dppF": "policy head helper: one float DPP step — called only from segMax / segSum / segScan and "
            "headField's exclusive shift, each of which checks the whole wave (LANE_AUDIT_WAVE)",
    "segMax": "policy head: DPP maximum over a quad / 16-lane row; headField calls it in uniform flow (k_head's loops "
              "test ballots and wave-uniform counts) with a select defined on every lane (-inf without a set bit)",
    "segSum": "policy head: as segMax, the operand a sum of selects (0 on lanes without a set bit or without a cell)",
    "segScan": "policy head: DPP running sum inside a quad / row, same call sites and operand as segSum",
    "headField": "policy head: the row_shr:1 of the running sum and the ballots sit outside every lane test; the "
                 "lane tests that follow (`ql == pick`, `set[k]`) only store or accumulate on their own lane",
    "dppD": "policy head helper: a double's two halves through one DPP step each — called only from waveSumD",
    "waveSumD": "policy head helper: wave_reduce's DPP chain and lane-63 read on doubles; its callers are k_head and "
                "k_head_packed",
    "k_head": "policy head: the kernel's last statement, after its chunk loop (whose `continue`, `while (m)` and "
              "bounds test ballots and kernel arguments: uniform); lp / ent are per-lane partial sums initialised to "
              "0 on every lane",
    "k_head_packed": "packed policy rows: as k_head, the kernel's last statement; the early return of a NaN row and the "
                     "chunk and round loops test the packed row's count and cells, read at wave-uniform addresses; the "
                     "rounds' headCell calls (segMax / segSum / ballots inside) sit in those uniform loops, a DPP row "
                     "without a candidate running them with every bit cleared.  k_head_pack's ballots (candidates, mask "
                     "bits) are in uniform flow too: its loops test ballots, the cap and kernel arguments",
    "k_obs_pack": "packed observation rows: no readlane or DPP — its cross-lane work is ballots (occupied cells, one per "
                  "plane 5.., the lossy flags) and mbcnt of a ballot, all at the chunk loop's top level or after it; the "
                  "loop's `continue`s and flushes test ballots, counts of ballots and kernel arguments (uniform), and each "
                  "ballot's operand is a select defined on every lane (false beyond the map).  The readers "
                  "(k_obs_unpack, k_obs_onehot_packed) have no cross-lane read",
    "k_lane_audit_probe": "the audit build's negative control (reads lane 40 from a branch only lanes 0-31 take)",
    "lrClosest": "LightRush: wave_min after the per-lane `for (o = lid() ...)` loop has reconverged; `best` starts at "
                 "INF on every lane; every caller passes wave-uniform arguments from uniform flow",
    "lrGameUsage": "LightRush: wave_sum of per-lane cost sums (0 on lanes without a PRODUCE) after the per-lane unit "
                   "loop; called once at the top of lightRush, in uniform flow",
    "lrAStarRun": "LightRush: wave_min of every lane's smallest open key (INF where a lane scanned nothing) in the pop "
               "loop, whose exits (open list empty, goal popped) test wave-uniform values (uni / the reduction)",
    "lrTranslate": "LightRush: wave_min of per-lane minima (INF elsewhere) over the bot memory in the entry loop; "
                   "`best == INF` and the `continue`s test wave-uniform values (uniu of LDS words, lrExecute's result)",
    "k_evaluate": "uniform `k < n` loop inside the uniform o0 loop; c / hpv / rv are initialised on every lane "
                  "(UC_DEAD / 0) before the `o < nu` loads",
}


def sites():
    """[(file, line, function, text)]"""
    out = []
    for src in SRCS:
        out += [(src,) + s for s in file_sites(os.path.join(CSRC, src))]
    return out


def file_sites(path):
    lines = open(path).read().split("\n")
    fn, out = None, []
    for i, l in enumerate(lines, 1):
        m = re.match(r"\s*(?:template\s*<[^>]*>\s*)?(?:static\s+)?(?:DEV|__global__)[^(]*?\b(\w+)\s*\(", l)
        if m and not l.strip().startswith("//"):
            fn = m.group(1)
            if fn == "__launch_bounds__":
                k = re.search(r"\)\s*void\s+(\w+)\s*\(", l)
                fn = k.group(1) if k else fn
        if "#define" in l or "DEV int rl(" in l or "DEV int rlAudit" in l:
            continue
        code = l.split("//")[0]
        if re.search(r"\brl\(|\bwave_(sum|min|incl_sum)\s*\(|\bwave_reduce\s*<|update_dpp\(|\bquadOr\(|\bdppF\s*<|\bseg(Max|Sum|Scan)\s*<|"
                     r"\bdppD\s*<|\bwaveSumD\(", code):
            out.append((i, fn, l.strip()))
    return out


def main():
    md = "--markdown" in sys.argv
    s = sites()
    missing = sorted({f for _, _, f, _ in s if f not in WHY})
    by = {}
    for src, i, f, _ in s:
        by.setdefault((src, f), []).append(i)
    if md:
        print("| function | file: lines | why the lanes read are active |")
        print("|---|---|---|")
        for (src, f), ls in by.items():
            print(f"| `{f}` | {src}: {', '.join(map(str, ls))} | {WHY.get(f, '**MISSING**')} |")
    else:
        for src, i, f, t in s:
            print(f"{src}:{i:<5d} {f:20s} {t[:100]}")
    if missing:
        print(f"sites in functions without a reason: {missing}", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
