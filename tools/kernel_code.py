#!/usr/bin/env python3
"""The kernels of a library, one line each: what a change that must not touch device code is checked against.

For every gfx950 code object of a libmrts*.so (or of a device-only object, `hipcc --cuda-device-only -c`), in file
order, and every kernel in it: symbol, size in bytes, SHA-256 of the function's bytes, and SHA-256 of its 64-byte
kernel descriptor with kernel_code_entry_byte_offset (bytes 16-23: the code's distance from the descriptor, which
moves when other kernels of the object change size) zeroed.  Two builds run the same kernels when their tables are
equal; `--diff A B` says where they are not (exit status 1), matching kernels by symbol whatever object they are in.
A kernel of equal size whose bytes differ is disassembled from both (llvm-objdump -d): if the two listings differ only
in the literal that an s_add_u32 / s_addc_u32 adds to an s_getpc_b64 result — a pc-relative address of data outside the
function, which moves with the function — the line says so, and that is no difference in what the kernel does.

Usage: python tools/kernel_code.py LIB            the table
       python tools/kernel_code.py --diff A B     compare two libraries [--sizes-only: symbols and sizes]
"""
import hashlib
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from microrts_amd import _lib  # noqa: E402


def kernels(path):
    """[(code object index, symbol, size, function sha256, masked descriptor sha256)], kernels in address order"""
    out = []
    for k, obj in enumerate(_lib.device_code_objects(path)):
        secs = _lib._elf_sections(obj)
        _, _, _, off, size, link, ent = next(s for s in secs if s[0] == ".symtab")
        stroff = secs[link][3]
        syms = {}
        for i in range(size // ent):
            name, info, _, shndx, value, ssize = struct.unpack_from("<IBBHQQ", obj, off + i * ent)
            if shndx == 0 or shndx >= 0xFF00:
                continue
            n = obj[stroff + name:obj.index(b"\0", stroff + name)].decode()
            addr, soff = secs[shndx][2], secs[shndx][3]
            syms[n] = (info & 15, value, obj[soff + value - addr:soff + value - addr + ssize])
        for n, (typ, value, code) in sorted(syms.items(), key=lambda kv: kv[1][1]):
            kd = syms.get(n + ".kd")
            if typ != 2 or kd is None:  # STT_FUNC with a kernel descriptor
                continue
            d = kd[2]
            assert len(d) == 64, f"{n}.kd: {len(d)} bytes"
            out.append((k, n, len(code), hashlib.sha256(code).hexdigest(), hashlib.sha256(d[:16] + bytes(8) + d[24:]).hexdigest()))
    return out


OBJDUMP = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump")


def pc_relative_only(a, b, ka, kb):
    """the differing instructions of kernel ka / kb (rows of kernels()) of libraries a / b, if every one of them is an
    s_add(c)_u32 of a literal within 3 instructions after an s_getpc_b64 — else None"""
    import re
    import subprocess
    import tempfile

    text = []
    for path, row in ((a, ka), (b, kb)):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(_lib.device_code_objects(path)[row[0]])
            f.flush()
            o = subprocess.check_output([OBJDUMP, "-d", f"--disassemble-symbols={row[1]}", f.name], text=True)
        text.append([ln.split("//")[0].strip() for ln in o.split("\n") if ln.startswith("\t")])
    if len(text[0]) != len(text[1]):
        return None
    kinds = {}
    for i, (x, y) in enumerate(zip(*text)):
        if x == y:
            continue
        mx, my = (re.fullmatch(r"(s_addc?_u32 s\d+, s\d+), 0x[0-9a-f]+", t) for t in (x, y))
        if not (mx and my and mx.group(1) == my.group(1) and any(t.startswith("s_getpc_b64") for t in text[0][max(0, i - 3):i])):
            return None
        kinds[x.split()[0]] = kinds.get(x.split()[0], 0) + 1
    return kinds


def diff(a, b, sizes_only):
    """the lines that say where two tables differ; empty = the same kernels"""
    ka, kb = {r[1]: r for r in kernels(a)}, {r[1]: r for r in kernels(b)}
    lines = [f"only in {a}: {n}" for n in ka if n not in kb] + [f"only in {b}: {n}" for n in kb if n not in ka]
    moved = []  # kernels whose only difference is a pc-relative literal
    for n in ka:
        if n not in kb:
            continue
        for what, i in (("size", 2), ("code", 3), ("descriptor", 4)):
            if ka[n][i] != kb[n][i] and not (sizes_only and i > 2):
                pc = pc_relative_only(a, b, ka[n], kb[n]) if i == 3 else None
                (moved if pc else lines).append(f"{what} differs: {n} ({ka[n][2]} / {kb[n][2]} bytes)" +
                                                (f" — pc-relative literals only: {pc}" if pc else ""))
                break
    return len(ka), len(kb), lines, moved


def main():
    args = [x for x in sys.argv[1:] if not x.startswith("--")]
    if "--diff" in sys.argv:
        na, nb, lines, moved = diff(args[0], args[1], "--sizes-only" in sys.argv)
        print(f"{na} / {nb} kernels, {len(lines)} differences, {len(moved)} moved; device code {_lib.device_code_sha256(args[0])} / "
              f"{_lib.device_code_sha256(args[1])}")
        print("\n".join(moved + lines))
        sys.exit(1 if lines else 0)
    for k, n, size, h, hd in kernels(args[0]):
        print(f"{k} {n} {size} {h} {hd}")


if __name__ == "__main__":
    main()
