"""What the CPU tests read out of the C headers: the entry points include/mrts.h declares, their full prototypes and
the comparison of a ctypes table with them, and the constants and one-line functions of
microrts_amd/csrc/mrts_internal.h.  Test infrastructure only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    """Every mrts_* function include/mrts.h declares, sorted."""
    txt = open(os.path.join(ROOT, "include", "mrts.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(mrts_[a-z0-9_]+)\s*\(", txt)))


def header_prototypes():
    """name -> (return type, [argument types]) of every function include/mrts.h declares, as C text without the
    parameter names ("const int32_t*", "uint64_t"; `(void)` is no arguments)."""
    txt = open(os.path.join(ROOT, "include", "mrts.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    txt = re.sub(r"^\s*#.*$", "", txt, flags=re.M)
    txt = re.sub(r'extern\s+"C"\s*\{', "", txt)
    txt = re.sub(r"\{[^{}]*\}", "", txt)  # struct and enum bodies
    out = {}
    for statement in txt.split(";"):
        m = re.match(r"\s*([\w\s\*]+?)\s*\b(mrts_[a-z0-9_]+)\s*\(([^()]*)\)\s*$", statement, flags=re.S)
        if not m:
            continue
        ret, name, args = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
        assert name not in out, f"{name} is declared twice"
        types = []
        for a in ([] if args in ("", "void") else args.split(",")):
            t = re.match(r"\s*(.*?[\s\*])\w+\s*$", a)  # everything before the parameter's name
            assert t, f"{name}: unnamed parameter {a!r}"
            types.append(re.sub(r"\s*\*", "*", t.group(1).strip()))
        out[name] = (re.sub(r"\s*\*", "*", ret), types)
    return out


def c_type_class(t, ret=False):
    """What a C type of the header is to a ctypes binding: "pointer", "int32" (`int` too), "uint32", "int64",
    "uint64"; for a return type also "const char*" (a string the binding decodes) and "void"."""
    if ret and t in ("const char*", "void"):
        return t
    if t.endswith("*"):
        return "pointer"
    return {"int": "int32", "int32_t": "int32", "uint32_t": "uint32", "int64_t": "int64", "uint64_t": "uint64"}[t]


def ctypes_class(t, ret=False):
    """c_type_class of a ctypes type of a binding (an argtypes entry or a restype)."""
    import ctypes

    if ret and t is None:
        return "void"
    if ret and t is ctypes.c_char_p:
        return "const char*"
    if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
        return "pointer"
    return {ctypes.c_int32: "int32", ctypes.c_uint32: "uint32", ctypes.c_int64: "int64", ctypes.c_uint64: "uint64"}[t]


def signature_mismatches(prototypes, table):
    """What differs between the header's prototypes and a binding's table name -> (argtypes, restype): a list of
    texts, empty when every prototype has its entry with the same number of arguments, the same class for each
    and the same return class."""
    bad = [f"{n}: not in the table" for n in prototypes if n not in table]
    bad += [f"{n}: not in the header" for n in table if n not in prototypes]
    for name, (ret, args) in prototypes.items():
        if name not in table:
            continue
        argtypes, restype = table[name]
        if len(argtypes) != len(args):
            bad.append(f"{name}: {len(argtypes)} arguments, the header has {len(args)}")
            continue
        for i, (c, t) in enumerate(zip(args, argtypes)):
            if c_type_class(c) != ctypes_class(t):
                bad.append(f"{name}: argument {i} is {ctypes_class(t)}, the header has {c}")
        if c_type_class(ret, ret=True) != ctypes_class(restype, ret=True):
            bad.append(f"{name}: returns {ctypes_class(restype, ret=True)}, the header has {ret}")
    return bad


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
