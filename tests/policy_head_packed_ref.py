"""Reference side of the packed policy rows' tests — test infrastructure.

A numpy packer written from the description in include/mrts.h ("Packed policy rows"): the words per candidate and
the action word's (shift, bits) pairs are read out of the header's text, so the header cannot drift from what the
kernels write without a test noticing.  Also the canonical dense form that unpack returns, and the synthetic rows the
GPU tests share."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_layout():
    """(words per candidate, [(shift, bits)] * 7, mask words) as include/mrts.h states them"""
    txt = open(os.path.join(ROOT, "include", "mrts.h")).read()
    sec = txt[txt.index("Packed policy rows"):]
    sec = re.sub(r"\s*\n \*\s*", " ", sec[:sec.index("*/")])
    cw = int(re.search(r"A packed row is 1 \+ cap \* (\d+) uint32 words", sec).group(1))
    assert int(re.search(r"in ascending cell order, (\d+) words each", sec).group(1)) == cw
    m = re.search(r"\(s_f, b_f\) = ((?:\(\d+,\d+\) ?){7})for f = 0\.\.6", sec)
    fields = [(int(a), int(b)) for a, b in re.findall(r"\((\d+),(\d+)\)", m.group(1))]
    lo, hi, nbits = re.search(r"words (\d+)\.\.(\d+): the K mask bits, bit j of the (\d+)", sec).groups()
    assert int(lo) == 2 and int(hi) == cw - 1 and int(nbits) == 32 * (cw - 2)
    for part in ("word 0: the row's candidate count", "word 0: the cell index", "word 1: the seven action components"):
        assert part in sec, part
    return cw, fields, cw - 2


def act_word(row, fields):
    w = 0
    for c, (s, b) in zip(row, fields):
        off = (1 << b) - 1
        w |= (int(c) if 0 <= int(c) < off else off) << s
    return w


def candidates(masks, source=None):
    """bool [n][HW]: the source bits when given, else mask byte 0 != 0"""
    n, HW, _ = masks.shape
    if source is None:
        return masks[:, :, 0] != 0
    s = np.asarray(source).view(np.uint32)
    c = np.arange(HW)
    return ((s[:, c >> 5] >> (c & 31).astype(np.uint32)) & 1) != 0


def pack_rows(masks, actions, cap, source=None):
    """masks uint8 [n][HW][K], actions int32 [n][HW][7] -> uint32 [n][1 + cap * cw], as the header describes"""
    cw, fields, mw = header_layout()
    n, HW, K = masks.shape
    assert K <= 32 * mw
    cand = candidates(masks, source)
    out = np.zeros((n, 1 + cap * cw), np.uint32)
    for r in range(n):
        cells = np.flatnonzero(cand[r])
        out[r, 0] = len(cells)
        for i, c in enumerate(cells[:cap]):
            o = 1 + i * cw
            out[r, o] = c
            out[r, o + 1] = act_word(actions[r, c], fields)
            for j in np.flatnonzero(masks[r, c]):
                out[r, o + 2 + j // 32] |= np.uint32(1) << np.uint32(j % 32)
    return out


def canonical(masks, actions, cap=None, source=None):
    """The dense form unpack returns: mask bytes 0 / 1 and action rows at candidate cells (the first cap of a row),
    components outside [0, 2^bits - 1) as -1; zeros elsewhere."""
    _, fields, _ = header_layout()
    cand = candidates(masks, source)
    if cap is not None:
        cand = cand & (np.cumsum(cand, 1) <= cap)
    m = ((masks != 0) & cand[:, :, None]).astype(np.uint8)
    a = actions.astype(np.int64)
    off = np.array([(1 << b) - 1 for _, b in fields])
    a = np.where((a >= 0) & (a < off), a, -1)
    return m, (a * cand[:, :, None]).astype(np.int32)


def _field_ranges(K, nt):
    return [(0, 6), (6, 10), (10, 14), (14, 18), (18, 22), (22, 22 + nt), (22 + nt, K - 1)]


def synthetic_rows(HW, K, nt, seed):
    """Rows that reach every path of the packed kernels.  Returns (masks uint8 [n][HW][K], actions int32 [n][HW][7],
    names): candidate cells get random mask bits (every field non-empty unless the row says otherwise) and, per
    field, a component on a set bit; every other cell gets junk bits (mask byte 0 clear) and a junk action row, which
    neither form may read."""
    rng = np.random.default_rng(seed)
    fr = _field_ranges(K, nt)
    last = HW - 1
    at = lambda c: c % HW  # noqa: E731 (a 4x4 map: cells 20, 41 and 33 fold onto 4, 9 and 1, the counts stay 4 and 5)
    rows = [("none", []), ("one", [min(5, last)]), ("four", [1, 7, at(20), at(41)]), ("five", [0, 3, 9, 10, at(33)]),
            ("chunk0", list(range(min(64, HW)))), ("all", list(range(HW))), ("empty_field", [2, min(50, last)]),
            ("off_mask", [4, 11]), ("minus_one_and_huge", [6, 12, 13]), ("tail", sorted({0, max(last - 1, 0), last}))]
    if HW > 64:
        rows.append(("boundary", [62, 63, 64, 65] + ([127, 128] if HW > 128 else [])))
        rows.append(("boundary5", [59, 60, 61, 62, 63, 64]))
    n = len(rows)
    masks = (rng.random((n, HW, K)) < 0.3).astype(np.uint8) * rng.choice(np.array([1, 2, 255], np.uint8), (n, HW, K))
    masks[:, :, 0] = 0
    actions = rng.integers(-5, 200, (n, HW, 7)).astype(np.int32)
    for r, (name, cells) in enumerate(rows):
        for c in cells:
            rec = (rng.random(K) < 0.5).astype(np.uint8)
            rec[0] = 1 + 254 * (c & 1)
            for f, (lo, hi) in enumerate(fr):
                if not rec[1 + lo:1 + hi].any():
                    rec[1 + rng.integers(lo, hi)] = 1
            if name == "empty_field":
                for f in (1, 5, 6) if c == 2 else (0,):
                    rec[1 + fr[f][0]:1 + fr[f][1]] = 0
            masks[r, c] = rec
            for f, (lo, hi) in enumerate(fr):
                on = np.flatnonzero(rec[1 + lo:1 + hi])
                actions[r, c, f] = rng.choice(on) if len(on) else 0
            if name == "off_mask" and c == 4:
                masks[r, c, 1 + 0], masks[r, c, 1 + 3] = 1, 0  # type 3 cleared in a non-empty type field
                actions[r, c, 0] = 3
            if name == "off_mask" and c == 11:
                actions[r, c, 6] = K  # beyond the attack window
            if name == "minus_one_and_huge":
                actions[r, c, {6: 0, 12: 2, 13: 6}[c]] = -1 if c != 12 else 1 << 30
                if c == 13:
                    actions[r, c, 5] = 1 << 30
    return masks, actions, [name for name, _ in rows]
