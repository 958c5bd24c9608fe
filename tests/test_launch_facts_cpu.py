"""The host-side facts a launch rests on, on the CPU: how much dynamic LDS a handle asks for, which instance of
k_env a launch runs, and whether the host may ask that instance for several steps (envIterable).  The library's own
functions are called through two internal probes (mrts_internal_lds_probe / mrts_internal_launch_probe in
mrts_kernels.hip, beside mrts_internal_steady_probe; not in include/mrts.h).  The expected values are the ones the
code had before the kernel file was split: the LDS table is the output of that commit's ldsBytes / lrLdsBytes
(compiled stand-alone), the selection table was read off its launchEnv and envIterable.  No GPU call is made.
"""
import ctypes
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (H, W, CAP, partial observability, a LightRush game) -> bytes.  Every map shape under maps/, CAP as mrts_create
# sizes it (H * W + max(64, H * W / 4)); LightRush up to LR_MAX_CELLS = 1024 cells.
LDS_BYTES = {
    (4, 4, 80, 0, 0): 3132, (4, 4, 80, 0, 1): 5584, (4, 4, 80, 1, 0): 3364, (4, 4, 80, 1, 1): 5824,
    (8, 8, 128, 0, 0): 4348, (8, 8, 128, 0, 1): 8652, (8, 8, 128, 1, 0): 4948, (8, 8, 128, 1, 1): 9260,
    (8, 9, 136, 0, 0): 4556, (8, 9, 136, 0, 1): 9168, (8, 9, 136, 1, 0): 4908, (8, 9, 136, 1, 1): 9520,
    (8, 16, 192, 0, 0): 5972, (8, 16, 192, 0, 1): 12748, (8, 16, 192, 1, 0): 6892, (8, 16, 192, 1, 1): 13660,
    (10, 10, 164, 0, 0): 5268, (10, 10, 164, 0, 1): 10968, (10, 10, 164, 1, 0): 5748, (10, 10, 164, 1, 1): 11448,
    (12, 12, 208, 0, 0): 6384, (12, 12, 208, 0, 1): 13772, (12, 12, 208, 1, 0): 7536, (12, 12, 208, 1, 1): 14924,
    (12, 14, 232, 0, 0): 6996, (12, 14, 232, 0, 1): 15324, (12, 14, 232, 1, 0): 7764, (12, 14, 232, 1, 1): 16092,
    (12, 16, 256, 0, 0): 7596, (12, 16, 256, 0, 1): 16828, (12, 16, 256, 1, 0): 8988, (12, 16, 256, 1, 1): 18220,
    (14, 15, 274, 0, 0): 8060, (14, 15, 274, 0, 1): 17992, (14, 15, 274, 1, 0): 9012, (14, 15, 274, 1, 1): 18952,
    (16, 16, 320, 0, 0): 10180, (16, 16, 320, 0, 1): 21884, (16, 16, 320, 1, 0): 11060, (16, 16, 320, 1, 1): 22764,
    (24, 24, 720, 0, 0): 19184, (24, 24, 720, 0, 1): 45448, (24, 24, 720, 1, 0): 22952, (24, 24, 720, 1, 1): 49224,
    (32, 32, 1280, 0, 0): 33128, (32, 32, 1280, 0, 1): 79784, (32, 32, 1280, 1, 0): 39464, (32, 32, 1280, 1, 1): 86120,
    (64, 64, 5120, 0, 0): 128752, (64, 64, 5120, 1, 0): 146160,
    (96, 128, 15360, 0, 0): 383744, (96, 128, 15360, 1, 0): 435968,
    (112, 128, 17920, 0, 0): 447488, (112, 128, 17920, 1, 0): 508416,
    (128, 96, 15360, 0, 0): 383736, (128, 96, 15360, 1, 0): 435960,
    (128, 128, 20480, 0, 0): 511232, (128, 128, 20480, 1, 0): 580864,
}

# EnvInst (mrts_kernels.hip) in its order, one letter each in the tables below
INSTANCES = ["STEADY16", "MULTI16", "STEP16", "HELP8", "MULTI8", "STEP8", "HELP32PO", "MULTI32PO", "STEP32PO", "STEP_LR", "STEP",
             "RESET_LR", "RESET", "PLAYOUT", "TRACE16", "TRACE8", "TRACE", "MASKS"]
LETTERS = "ABCDEFGHIJKLMNOPQR"
MULTI = {"STEADY16", "MULTI16", "HELP8", "MULTI8", "HELP32PO", "MULTI32PO"}
MODE_STEP, MODE_RESET, MODE_MASKS, MODE_PLAYOUT, MODE_TRACE = range(5)
# MODE_STEP launches in the order of the strings below: (n_iter, rows, uniform rows, masks, obs)
STEP_LAUNCHES = list(itertools.product((1, 20), (0, 1), (0, 1), (0, 1), (0, 1)))
# (handle, (H, W, CAP, po, K, ntypes, maxAttackRadius, every game self-play, a LightRush game),
#  the instance of each of STEP_LAUNCHES, the instances of MODE_RESET / MASKS / PLAYOUT / TRACE, envIterable)
SELECTION = [
    ("16x16", (16, 16, 320, 0, 79, 7, 7, 1, 0), "CCCCCCCCKKKKKKKKBBBABBBBKKKKKKKK", "MRNO", True),
    ("8x8", (8, 8, 128, 0, 79, 7, 7, 1, 0), "FFFFFFFFKKKKKKKKEEEEDDEEKKKKKKKK", "MRNP", True),
    ("32x32 PO", (32, 32, 320, 1, 79, 7, 7, 1, 0), "IIIIIIIIKKKKKKKKHGHGHGHGKKKKKKKK", "MRNQ", True),
    ("16x16, H + 1", (17, 16, 320, 0, 79, 7, 7, 1, 0), "K" * 32, "MRNQ", False),
    ("16x16, W + 1", (16, 17, 320, 0, 79, 7, 7, 1, 0), "K" * 32, "MRNQ", False),
    ("16x16, CAP + 1", (16, 16, 321, 0, 79, 7, 7, 1, 0), "K" * 32, "MRNQ", False),
    ("16x16, po", (16, 16, 320, 1, 79, 7, 7, 1, 0), "K" * 32, "MRNQ", False),
    ("16x16, K + 1", (16, 16, 320, 0, 80, 7, 7, 1, 0), "K" * 32, "MRNQ", False),
    ("16x16, ntypes + 1", (16, 16, 320, 0, 79, 8, 7, 1, 0), "K" * 32, "MRNQ", False),
    ("16x16, radius - 1", (16, 16, 320, 0, 79, 7, 6, 1, 0), "K" * 32, "MRNQ", False),
    ("16x16, a bot game", (16, 16, 320, 0, 79, 7, 7, 0, 0), "K" * 32, "MRNO", False),  # MODE_TRACE ignores the games' kinds
    ("16x16 with a LightRush game", (16, 16, 320, 0, 79, 7, 7, 0, 1), "J" * 32, "LRNO", False),
    ("8x8, CAP + 1", (8, 8, 129, 0, 79, 7, 7, 1, 0), "K" * 32, "MRNQ", False),
    ("32x32 PO, full observability", (32, 32, 320, 0, 79, 7, 7, 1, 0), "K" * 32, "MRNQ", False),
]


@pytest.fixture(scope="module")
def lib():
    from microrts_amd import _lib

    return _lib.load()


def test_handle_lds_bytes_are_the_parents(lib):
    probe = lib.mrts_internal_lds_probe
    probe.argtypes, probe.restype = [ctypes.c_int] * 5, ctypes.c_int
    shapes = set()
    for d, _, files in os.walk(os.path.join(ROOT, "maps")):
        for fn in files:
            if fn.endswith(".xml"):
                head = open(os.path.join(d, fn), errors="replace").read(4096)
                shapes.add((int(re.search(r'height="(\d+)"', head).group(1)), int(re.search(r'width="(\d+)"', head).group(1))))
    assert shapes == {k[:2] for k in LDS_BYTES} and len(shapes) == 17, "the table covers every map shape under maps/"
    for (H, W, CAP, po, lr), want in LDS_BYTES.items():
        assert CAP == H * W + max(64, H * W // 4)
        assert probe(H * W, W, CAP, po, lr) == want, f"{H}x{W} CAP {CAP} po {po} LightRush {lr}"
    for H, W in shapes:  # both observabilities, and LightRush wherever a handle can have it
        assert all(((H, W, H * W + max(64, H * W // 4), po, lr) in LDS_BYTES) == (not lr or H * W <= 1024)
                   for po in (0, 1) for lr in (0, 1))


def test_instance_selection_is_the_parents(lib):
    probe = lib.mrts_internal_launch_probe
    probe.argtypes, probe.restype = [ctypes.c_int] * 15, ctypes.c_int
    for what, handle, step, other, iterable in SELECTION:
        got = "".join(LETTERS[probe(*handle, MODE_STEP, *launch) & 255] for launch in STEP_LAUNCHES)
        assert got == step, f"{what}: MODE_STEP over (n_iter, rows, uniform, masks, obs)"
        got = "".join(LETTERS[probe(*handle, mode, 1, 0, 0, 1, 1) & 255]
                      for mode in (MODE_RESET, MODE_MASKS, MODE_PLAYOUT, MODE_TRACE))
        assert got == other, f"{what}: MODE_RESET / MASKS / PLAYOUT / TRACE"
        assert bool(probe(*handle, MODE_STEP, 1, 0, 0, 1, 1) >> 8) == iterable, f"{what}: envIterable"


def test_iterable_exactly_where_a_multi_step_instance_exists(lib):
    """The host raises n_iter above 1 on envIterable alone: it must hold exactly for the handles that some launch
    with n_iter > 1 sends to a MULTI instance, and such a launch without rows must never reach a single-step one."""
    probe = lib.mrts_internal_launch_probe
    probe.argtypes, probe.restype = [ctypes.c_int] * 15, ctypes.c_int
    for what, handle, _, _, _ in SELECTION:
        picked = {launch: INSTANCES[probe(*handle, MODE_STEP, *launch) & 255] for launch in STEP_LAUNCHES if launch[0] > 1}
        iterable = bool(probe(*handle, MODE_STEP, 20, 0, 0, 1, 1) >> 8)
        assert iterable == any(i in MULTI for i in picked.values()), what
        if iterable:
            assert all(i in MULTI for launch, i in picked.items() if not launch[1]), f"{what}: {picked}"


def test_device_code_hash_visits_every_unit():
    """device_code_sha256 covers the gfx950 code object of every .hip unit the library is linked from."""
    import sys

    from microrts_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmrts.so is not built")
    sys.path.insert(0, ROOT)
    from tools import kernel_code

    units = [fn for fn in os.listdir(os.path.join(ROOT, "microrts_amd", "csrc")) if fn.endswith(".hip")]
    objs = _lib.device_code_objects()
    assert len(objs) == len(units) == 3
    rows = kernel_code.kernels(_lib.LIB_PATH)
    assert {r[0] for r in rows} == {0, 1, 2}, "kernels in every code object"
    for name in ("k_env", "k_head", "k_onehot"):
        assert any(name in r[1] for r in rows), name
