// mrts_ablate.h — the phases of the ablation build (-DMRTS_ABLATE, `make ablate`), one row each: the only place
// that numbers or names them.  mrts_kernels.hip makes the AB_* enum from it, mrts_host.cpp exports it
// (mrts_ablate_phase), and the tools and tests/test_gpu_ablate.py read names, kinds and bits from that export.
//
//   X(enum name without AB_, bit of the flag word, kind, the name the tools print, its name on the steady instance)
//
// Kinds: AGAIN runs the phase once more and leaves every output as it was (tests/test_gpu_ablate.py holds all of
// these set against the product library); SKIP leaves something out, so outputs change; COUNT adds to the
// diagnostics counters (mrts_get_dbg).  A printed name in parentheses keeps the row out of the tools' default
// selection.  The last column is the row's name where the steady 16x16 instance prices something else under the
// same bit, else nullptr: its mask pass (writeMasksSteady) is one list of quads for own idle units
// and vacated cells, so there `record` / `SKIP records` are the quad stores of every entry, vacated cells' zero
// records included; `gone` is the scan that counts the vacated cells alone — their listing, records and zero rows
// ride the unit pass and cannot be doubled apart from it; `maskbits` doubles the quads' bits (four lanes per
// entry) without the hand-off into the quads.
//
// Rows 16-17 skip the observation / the mask record stores (nothing the step reads back).  Rows 18-23 split the PO
// observation: everything but the stores (values kept alive), only the stores (zeros), and pieces skipped — sight-disk
// painting, the last-writer cell map, the render record, the snapshots.  Rows 24-28 are the step's
// glue: the forwarded row's decode (decodeFwd on a launch's first step, else the steady instance's sampledDec +
// unpack), nextStep, the priority / SIMD-rank block at the top of the iteration, writeMasksLanes' set-up before
// maskTables, and cycleLanes' execute loop WITHOUT the executes (not idempotent): the pick of each ready item and its
// lane reads.  Rows 30-31 (§5r), the steady instance: cycleLanes' lane-parallel MOVE pass and the step's reward / done
// stores, each once more.  Row 32, the steady instance only: compact() once more in a step with a death.
#pragma once
#define MRTS_AB_PHASES(X)                                                                   \
    X(LOAD, 0, AGAIN, "load", nullptr)                                                      \
    X(OBS, 1, AGAIN, "obs", nullptr)                                                        \
    X(STORE, 2, AGAIN, "store", nullptr)                                                    \
    X(MASKBITS, 3, AGAIN, "maskbits", "maskbits (quads, no hand-off)")                      \
    X(RECORD, 4, AGAIN, "record", "record (units + vacated cells)")                         \
    X(POLICY, 5, AGAIN, "policy", nullptr)                                                  \
    X(ACCEPT, 6, AGAIN, "accept", nullptr)                                                  \
    X(LEGAL, 7, AGAIN, "legality", nullptr)                                                 \
    X(OUTCOME, 8, AGAIN, "outcome+rewards", nullptr)                                        \
    X(INDEX, 9, AGAIN, "index", nullptr)                                                    \
    X(GONE, 10, AGAIN, "gone", "gone (the count alone)")                                    \
    X(TABLES, 11, AGAIN, "tables", nullptr)                                                 \
    X(RANK, 12, AGAIN, "rank", nullptr)                                                     \
    X(DECODE, 13, AGAIN, "decode", nullptr)                                                 \
    X(ISSUE, 14, AGAIN, "issue", nullptr)                                                   \
    X(CYCLERANK, 15, AGAIN, "cyclerank", nullptr)                                           \
    X(SKIP_OBS, 16, SKIP, "SKIP obs", nullptr)                                              \
    X(SKIP_RECORD, 17, SKIP, "SKIP records", "SKIP records (units + vacated cells)")        \
    X(PO_NOSTORE, 18, SKIP, "SKIP PO render pass", nullptr)                                 \
    X(PO_ZEROSTORE, 19, SKIP, "PO render without its stores", nullptr)                      \
    X(PO_NOPAINT, 20, SKIP, "SKIP PO disk painting", nullptr)                               \
    X(PO_NOSCELL, 21, SKIP, "SKIP PO cell map", nullptr)                                    \
    X(PO_NORECORD, 22, SKIP, "SKIP PO render record", nullptr)                              \
    X(PO_NOSNAPSHOT, 23, SKIP, "(snapshot)", nullptr)                                       \
    X(DECFWD, 24, AGAIN, "decodefwd", nullptr)                                              \
    X(NEXTSTEP, 25, AGAIN, "nextstep", nullptr)                                             \
    X(PRIO, 26, AGAIN, "prio+rank", nullptr)                                                \
    X(MASKSETUP, 27, AGAIN, "masksetup", nullptr)                                           \
    X(EXECLOOP, 28, AGAIN, "execloop (picks only)", nullptr)                                \
    X(COUNT, 29, COUNT, "(render-item counters)", nullptr)                                  \
    X(MOVEBATCH, 30, AGAIN, "movebatch", nullptr)                                           \
    X(REWARD, 31, AGAIN, "rewardstores", nullptr)                                           \
    X(COMPACT_STEADY, 32, AGAIN, "compact (steps with a death)", nullptr)
