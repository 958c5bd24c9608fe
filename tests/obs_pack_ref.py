"""Packed observation rows in numpy, written from the layout in include/mrts.h ("Packed observation rows"), not from
the kernels: pack, unpack, the MicroRTS-Py one-hot encoding, and the synthetic rows the CPU and GPU tests share.

A row of an observation int32 [C][H*W] at capacity cap is 1 + 2 * cap + (C - 5) * ceil(H*W / 32) uint32 words:
  word 0      n | lossy << 31, n = cells where any of planes 0-4 (hp, resources, owner, type, action) is non-zero;
              lossy: n > cap, a kept value clamped, or a value of planes 5.. neither 0 nor 1
  2 per cell  the first min(n, cap) such cells, ascending: cell | owner << 16 | action << 18 | type << 21, then
              (hp & 0xFFFF) | resources << 16; values clamped to their fields (owner 2 bits, action 3, type 5, hp
              int16, resources uint16); zero words after the last kept cell
  bitmaps     per plane 5..C-1, bit c % 32 of word c / 32 set <=> the plane is non-zero at cell c"""
import numpy as np

LOSSY = 1 << 31
# field ranges of planes 0-4: hp, resources, owner, type, action
RANGES = [(-32768, 32767), (0, 65535), (0, 3), (0, 31), (0, 7)]


def words(C, HW, cap):
    return 1 + 2 * cap + (C - 5) * ((HW + 31) // 32)


def pack(obs, cap):
    """obs int [n][C][H][W] (or [n][C][H*W]) -> uint32 [n][words]"""
    obs = np.asarray(obs)
    n, C = obs.shape[:2]
    o = obs.reshape(n, C, -1).astype(np.int64)
    HW = o.shape[2]
    MW = (HW + 31) // 32
    out = np.zeros((n, words(C, HW, cap)), np.uint64)
    for r in range(n):
        occ = np.flatnonzero((o[r, :5] != 0).any(axis=0))
        lossy = len(occ) > cap
        for i, c in enumerate(occ[:cap]):
            v = []
            for p, (lo, hi) in enumerate(RANGES):
                x = int(o[r, p, c])
                y = min(max(x, lo), hi)
                lossy |= y != x
                v.append(y)
            hp, res, owner, typ, act = v
            out[r, 1 + 2 * i] = int(c) | owner << 16 | act << 18 | typ << 21
            out[r, 2 + 2 * i] = (hp & 0xFFFF) | res << 16
        for p in range(5, C):
            lossy |= bool(((o[r, p] != 0) & (o[r, p] != 1)).any())
            bits = np.zeros(32 * MW, np.uint8)
            bits[:HW] = o[r, p] != 0
            at = 1 + 2 * cap + (p - 5) * MW
            out[r, at:at + MW] = np.packbits(bits, bitorder="little").view("<u4")
        out[r, 0] = len(occ) | (LOSSY if lossy else 0)
    return out.astype(np.uint32)


def unpack(rows, C, H, W, cap):
    """uint32 [n][words] -> int32 [n][C][H][W]: the kept, clamped content (a stored count above cap reads cap cells, a
    stored cell outside the map is skipped)"""
    rows = np.asarray(rows).astype(np.int64)
    n, HW = rows.shape[0], H * W
    MW = (HW + 31) // 32
    assert rows.shape[1] == words(C, HW, cap)
    o = np.zeros((n, C, HW), np.int32)
    for r in range(n):
        for i in range(min(int(rows[r, 0]) & (LOSSY - 1), cap)):
            a, b = int(rows[r, 1 + 2 * i]), int(rows[r, 2 + 2 * i])
            c = a & 0xFFFF
            if c >= HW:
                continue
            hp = b & 0xFFFF
            o[r, 0, c] = hp - 65536 if hp >= 32768 else hp
            o[r, 1, c] = b >> 16
            o[r, 2, c] = (a >> 16) & 3
            o[r, 3, c] = (a >> 21) & 31
            o[r, 4, c] = (a >> 18) & 7
        for p in range(5, C):
            at = 1 + 2 * cap + (p - 5) * MW
            o[r, p] = np.unpackbits(rows[r, at:at + MW].astype("<u4").view(np.uint8), bitorder="little")[:HW]
    return o.reshape(n, C, H, W)


def onehot_sizes(C, ntypes):
    return ([5, 5, 3, ntypes + 1, 6, 2] + [2] * (C - 6))[:C]


def onehot(obs, ntypes):
    """gym_microrts `_encode_obs`: clip plane p to [0, n_p - 1], one-hot, channels last: uint8 [n][H][W][F]"""
    obs = np.asarray(obs)
    n, C, H, W = obs.shape
    sizes = onehot_sizes(C, ntypes)
    out = np.zeros((n, H, W, sum(sizes)), np.uint8)
    f = 0
    for p, s in enumerate(sizes):
        v = np.clip(obs[:, p], 0, s - 1)
        for k in range(s):
            out[:, :, :, f + k] = v == k
        f += s
    return out


def synthetic_cap(H, W):
    """the capacity the synthetic rows are built around: below H*W, so that cap + 1 cells exist"""
    return min(H * W - 1, 6)


def synthetic_rows(H, W, C, seed):
    """(obs int32 [n][C][H][W], names, info): info[name] = (n occupied, clamped, other) — `clamped`: a value of
    planes 0-4 leaves its field (flagged at any cap that keeps its cell), `other`: a plane 5.. value that is neither
    0 nor 1 (flagged at any cap).  Rows around synthetic_cap(H, W): at that cap "exactly_cap" is whole and
    "cap_plus_1" and "every_cell" are cut."""
    HW, cap = H * W, synthetic_cap(H, W)
    g = np.random.default_rng(seed)
    rows, names, info = [], [], {}

    def unit(o, c, hp=1, res=0, owner=1, typ=3, act=0):
        o[0, c], o[1, c], o[2, c], o[3, c], o[4, c] = hp, res, owner, typ, act

    def add(name, fill, clamped=False, other=False, planes=True):
        o = np.zeros((C, HW), np.int64)
        if planes:
            o[5:] = g.integers(0, 2, (C - 5, HW))
        fill(o)
        n = int((o[:5] != 0).any(axis=0).sum())
        rows.append(o)
        names.append(name)
        info[name] = (n, clamped, other)

    def some(k):
        def fill(o):
            for c in sorted(g.choice(HW, k, replace=False)):
                unit(o, c, hp=int(g.integers(1, 5)), res=int(g.integers(0, 30)), owner=int(g.integers(0, 3)),
                     typ=int(g.integers(0, 7)), act=int(g.integers(0, 6)))
        return fill

    add("empty", lambda o: None, planes=False)
    add("cell_0", lambda o: unit(o, 0))
    add("cell_last", lambda o: unit(o, HW - 1, hp=4, res=7, owner=2, typ=6, act=5))
    if HW > 64:
        add("cells_63_64", lambda o: (unit(o, 63), unit(o, 64, owner=2)))
    if HW > 256:
        add("cells_255_256", lambda o: (unit(o, 255), unit(o, 256, owner=2)))
    add("exactly_cap", some(cap))
    add("cap_plus_1", some(cap + 1))

    def every(o):
        for c in range(HW):
            unit(o, c, hp=1 + c % 4, res=c % 3, owner=c % 3, typ=c % 7, act=c % 6)
    add("every_cell", every)
    add("only_plane_4", lambda o: unit(o, HW // 2, hp=0, res=0, owner=0, typ=0, act=2))
    c = HW // 3
    for name, kw, clamped in [
            ("hp_-1", dict(hp=-1), False), ("hp_-32768", dict(hp=-32768), False), ("hp_32767", dict(hp=32767), False),
            ("hp_32768", dict(hp=32768), True), ("hp_-32769", dict(hp=-32769), True),
            ("res_65535", dict(res=65535), False), ("res_65536", dict(res=65536), True), ("res_-1", dict(res=-1), True),
            ("owner_3", dict(owner=3), False), ("owner_4", dict(owner=4), True),
            ("action_7", dict(act=7), False), ("action_8", dict(act=8), True),
            ("type_31", dict(typ=31), False), ("type_32", dict(typ=32), True)]:
        add(name, lambda o, kw=kw: unit(o, c, **kw), clamped=clamped)

    def terrain2(o):
        unit(o, 1)
        o[5, HW - 1] = 2
    add("terrain_2", terrain2, other=True)
    return np.stack(rows).reshape(len(rows), C, H, W).astype(np.int32), names, info


def flagged(info, names, cap):
    """which synthetic rows carry the lossy flag at `cap` — a clamped value only where its cell is kept, which it is
    in every synthetic row with one (a single unit)"""
    return np.array([info[k][0] > cap or info[k][1] or info[k][2] for k in names])
