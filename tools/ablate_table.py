"""The ablation build for the tools and tests/test_gpu_ablate.py: the library handle with its diagnostic prototypes
set, and its table of phases as the library itself exports it (mrts_ablate_phase; the rows of
microrts_amd/csrc/mrts_ablate.h) — nothing here or in a tool numbers or names a bit."""
import collections
import ctypes
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "microrts_amd", "libmrts_ablate.so")  # make -C microrts_amd/csrc ablate

# kind: "AGAIN" (the phase once more, outputs unchanged), "SKIP" (outputs change) or "COUNT" (diagnostics counters);
# steady_name: the row's name on the steady 16x16 instance (= name where the table gives none)
Phase = collections.namedtuple("Phase", "bit enum kind name steady_name")


def load(path=LIB):
    """(library, [Phase]) of the ablation build at `path`; a process loads one library (microrts_amd._lib)"""
    from microrts_amd import _lib

    L = _lib.load(path)
    L.mrts_set_ablate.argtypes = [ctypes.c_ulonglong]
    L.mrts_get_dbg.argtypes = [ctypes.c_void_p, ctypes.c_int]
    cp = ctypes.POINTER(ctypes.c_char_p)
    L.mrts_ablate_phase.argtypes = [ctypes.c_int, cp, cp, cp, cp]
    phases = []
    for bit in range(64):
        en, kind, name, steady = (ctypes.c_char_p() for _ in range(4))
        if L.mrts_ablate_phase(bit, ctypes.byref(en), ctypes.byref(kind), ctypes.byref(name), ctypes.byref(steady)) == 0:
            phases.append(Phase(bit, en.value.decode(), kind.value.decode(), name.value.decode(),
                                (steady.value or name.value).decode()))
    return L, phases


def mask(phases):
    """the flag word with these phases' bits set"""
    return sum(1 << p.bit for p in phases)


def by_enum(phases, enum):
    return next(p for p in phases if p.enum == enum)


def selection(phases, spec=None):
    """The phases a tool runs: those `spec` lists (comma-separated enum names or bit numbers, the tools' BITS), or the
    default selection — every row whose printed name is not in parentheses"""
    if not spec:
        return [p for p in phases if not p.name.startswith("(")]
    want = spec.split(",")
    return [p for p in phases if p.enum in want or str(p.bit) in want]
