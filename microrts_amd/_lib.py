"""ctypes binding of libmrts.so (include/mrts.h).  The product path is GPU-only: if the HIP
library is missing this module raises — there is no CPU fallback."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MRTS_LIB_PATH") or os.path.join(HERE, "libmrts.so")  # override: diagnostics builds only

MRTS_BOT_PASSIVE, MRTS_BOT_RANDOM_BIASED, MRTS_BOT_LIGHT_RUSH = 0, 1, 2
MRTS_MAX_HORIZON = 65536
MRTS_LOGITS_F32, MRTS_LOGITS_BF16, MRTS_LOGITS_F16 = 0, 1, 2  # the logits' element type of the policy head's typed calls
# a_rfs names (src/ai/reward/*.java) -> MRTS_RF_* ids
REWARD_FUNCTIONS = {"WinLossRewardFunction": 0, "ResourceGatherRewardFunction": 1, "ProduceWorkerRewardFunction": 2,
                    "ProduceBuildingRewardFunction": 3, "AttackRewardFunction": 4, "ProduceCombatUnitRewardFunction": 5,
                    "CloserToEnemyBaseRewardFunction": 6, "CloserToEnemyUnitRewardFunction": 7}
ERR_BITS = {
    1 << 0: "CAPACITY", 1 << 1: "ADDUNIT", 1 << 2: "PRODUCE_TYPE", 1 << 3: "OLDER_CONFLICT",
    1 << 4: "NEG_RESOURCES", 1 << 5: "MOVE_COLLISION", 1 << 6: "RECORD",
}


def err_bit(name):
    """The MRTS_ERR_* bit that ERR_BITS names `name`"""
    return next(bit for bit, n in ERR_BITS.items() if n == name)


def _elf_sections(obj):
    """[(name, type, address, offset, size, link, entry size)] of a 64-bit little-endian ELF image, by section index"""
    import struct

    shoff = struct.unpack_from("<Q", obj, 0x28)[0]
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", obj, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", obj, shoff + i * shentsize) for i in range(shnum)]
    stroff = secs[shstrndx][4]
    return [(obj[stroff + s[0]:obj.index(b"\0", stroff + s[0])].decode(), s[1], s[3], s[4], s[5], s[6], s[9]) for s in secs]


def _code_sections(obj):
    """The .text and .rodata sections (the kernels' machine code and kernel descriptors) of an amdgcn code
    object, concatenated: what the kernels run, without the symbol tables (hipcc's per-compile __hip_cuid_*
    symbol differs between builds of the same source under different -D flags)."""
    secs = {s[0]: s for s in _elf_sections(obj)}
    if ".text" not in secs:
        raise RuntimeError("amdgcn code object without .text")
    return b"".join(obj[secs[n][3]:secs[n][3] + secs[n][4]] for n in (".text", ".rodata") if n in secs)


def device_code_objects(path=None):
    """The gfx950 code objects of libmrts.so, in file order: the library is linked from several HIP objects
    (csrc/*.hip), each of which brings an offload bundle of its own into .hip_fatbin (bundles are 4 KiB-aligned;
    an object without device code brings an entry with no bytes).  Also takes a bare code object (a device-only
    compile)."""
    import struct

    data = open(path or LIB_PATH, "rb").read()
    secs = {s[0]: s for s in _elf_sections(data)}
    if ".hip_fatbin" not in secs:
        if struct.unpack_from("<H", data, 0x12)[0] == 224:  # EM_AMDGPU
            return [data]
        raise RuntimeError(f"{path or LIB_PATH}: no .hip_fatbin")
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    b = data[secs[".hip_fatbin"][3]:secs[".hip_fatbin"][3] + secs[".hip_fatbin"][4]]
    out, at = [], b.find(magic)
    while at >= 0:
        n, p = struct.unpack_from("<Q", b, at + 24)[0], at + 32
        end = p
        for _ in range(n):
            eoff, esize, tl = struct.unpack_from("<QQQ", b, p)
            p += 24
            triple = b[p:p + tl].decode()
            p += tl
            end = max(end, at + eoff + esize)
            if "amdgcn" in triple and esize:
                out.append(b[at + eoff:at + eoff + esize])
        at = b.find(magic, max(p, end))  # the next bundle, past this one's entries
    if not out:
        raise RuntimeError(f"{path or LIB_PATH}: no amdgcn code object in .hip_fatbin")
    return out


def device_code_sha256(path=None):
    """SHA-256 of the gfx950 code inside libmrts.so: the .text and .rodata — the kernels' machine code and
    descriptors — of every code object (device_code_objects), in file order.  Counter files (profiles/pmc_*.json)
    name the code they describe with it, so a host-only change to the library keeps them valid and any change to
    any kernel voids them."""
    import hashlib

    return hashlib.sha256(b"".join(_code_sections(o) for o in device_code_objects(path))).hexdigest()


class MrtsConfig(ctypes.Structure):
    _fields_ = [
        ("n_selfplay_slots", ctypes.c_int32),
        ("n_bot_envs", ctypes.c_int32),
        ("max_steps", ctypes.c_int32),
        ("partial_obs", ctypes.c_int32),
        ("utt_version", ctypes.c_int32),
        ("conflict_policy", ctypes.c_int32),
        ("bot_kinds", ctypes.POINTER(ctypes.c_int32)),
        ("ai1_kinds", ctypes.POINTER(ctypes.c_int32)),
        ("map_paths", ctypes.POINTER(ctypes.c_char_p)),
        ("device", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
        ("slot_id_base", ctypes.c_int32),
        ("mask_delta", ctypes.c_int32),
        ("reward_kinds", ctypes.POINTER(ctypes.c_int32)),
        ("n_rewards", ctypes.c_int32),
        ("forward_model", ctypes.c_int32),
        ("utt_json", ctypes.c_char_p),
        ("max_units", ctypes.c_int32),
    ]


class MrtsResponses(ctypes.Structure):
    _fields_ = [
        ("obs", ctypes.POINTER(ctypes.c_int32)),
        ("reward", ctypes.POINTER(ctypes.c_double)),
        ("done", ctypes.POINTER(ctypes.c_uint8)),
    ]


_P, _C, _INT = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int
_I32, _U32, _I64, _U64 = ctypes.c_int32, ctypes.c_uint32, ctypes.c_int64, ctypes.c_uint64
_PP, _PI64 = ctypes.POINTER(_P), ctypes.POINTER(_I64)
_CFG, _RESP = ctypes.POINTER(MrtsConfig), ctypes.POINTER(MrtsResponses)
_BUFS = [_P, _P, _P, _P, _P]  # d_actions, d_players, d_obs, d_reward, d_done
# every prototype of include/mrts.h: name -> (argument types, return type); load() sets them, and
# tests/test_abi_cpu.py holds each entry against the header's prototype
SIGNATURES = {
    "mrts_create": ([_CFG, _PP], _INT),
    "mrts_dims": ([_P, _P, _P, _P, _P, _P], _INT),
    "mrts_reset": ([_P, _P, _RESP], _INT),
    "mrts_step": ([_P, _P, _P, _RESP], _INT),
    "mrts_get_masks": ([_P, _I32, _P], _INT),
    "mrts_step_rows": ([_P, _P, _I32, _P, _RESP], _INT),
    "mrts_get_masks_i32": ([_P, _I32, _P], _INT),
    "mrts_get_masks_host": ([_P, _I32, _PP], _INT),
    "mrts_get_masks_i32_host": ([_P, _I32, _PP], _INT),
    "mrts_reset_dev": ([_P, _P, _P, _P, _P, _P, _I32, _P], _INT),
    "mrts_step_dev": ([_P, *_BUFS, _P, _I32, _P], _INT),
    "mrts_get_masks_dev": ([_P, _I32, _P, _P], _INT),
    "mrts_step_rows_dev": ([_P, _P, _I32, _P, _P, _P, _P, _P, _I32, _P], _INT),
    "mrts_get_masks_i32_dev": ([_P, _I32, _P, _P], _INT),
    "mrts_policy_dev": ([_P, _P, _P, _U64, _U32, _P, _P], _INT),
    "mrts_step_fused_dev": ([_P, *_BUFS, _P, _I32, _U64, _U32, _P], _INT),
    "mrts_rollout_fused_dev": ([_P, *_BUFS, _P, _I32, _U64, _U32, _I32, _P], _INT),
    "mrts_rccl_unique_id": ([_C, _P], _INT),
    "mrts_exchange_init": ([_P, _C, _I32, _I32, _P], _INT),
    "mrts_exchange_init_loopback": ([_P, _I32, _I32], _INT),
    "mrts_rollout_fused_exchange_dev": ([_P, *_BUFS, _P, _I32, _U64, _U32, _I32, _P, _P, _P, _P], _INT),
    "mrts_set_exchange_bytes": ([_P, _I32], _INT),
    "mrts_rollout_uniform_exchange_dev": ([_P, *_BUFS, _U64, _U32, _I32, _P, _P, _P, _P], _INT),
    "mrts_set_records": ([_P, _I32, _I32], _INT),
    "mrts_rollout_fused_records_dev": ([_P, *_BUFS, _P, _I32, _U64, _U32, _I32, _P, _P, _P], _INT),
    "mrts_rollout_uniform_records_dev": ([_P, *_BUFS, _U64, _U32, _I32, _P, _P, _P], _INT),
    "mrts_record_words": ([_P], _I32),
    "mrts_render_records_dev": ([_P, _P, _I64, _I32, _I64, _P, _I32, _P], _INT),
    "mrts_render_records_onehot_dev": ([_P, _P, _I64, _I32, _I64, _P, _P, _I32, _P, _P], _INT),
    "mrts_render_status": ([_P], _INT),
    "mrts_set_step_responses": ([_P, _P, _P, _I32], _INT),
    "mrts_capture_begin": ([_P, _P], _INT),
    "mrts_capture_end": ([_P, _P], _INT),
    "mrts_replay": ([_P, _P], _INT),
    "mrts_set_rollout_events": ([_P, _P, _P], _INT),
    "mrts_set_obs16": ([_P, _P], _INT),
    "mrts_set_multi_step": ([_P, _I32], _INT),
    "mrts_multi_step_capable": ([_P], _INT),
    "mrts_policy_uniform_dev": ([_P, _U64, _U32, _P, _P], _INT),
    "mrts_step_uniform_dev": ([_P, *_BUFS, _P, _I32, _U64, _U32, _P], _INT),
    "mrts_rollout_uniform_dev": ([_P, *_BUFS, _U64, _U32, _I32, _I32, _P], _INT),
    "mrts_set_obs_delta": ([_P, _I32], _INT),
    "mrts_obs_invalidate": ([_P], _INT),
    "mrts_policy_invalidate": ([_P], _INT),
    "mrts_policy_head_sample_dev": ([_P, _P, _P, _P, _U64, _U32, _P, _P, _P, _P], _INT),
    "mrts_policy_head_score_dev": ([_P, _I32, _P, _P, _P, _P, _P, _P], _INT),
    "mrts_policy_head_grad_dev": ([_P, _I32, _P, _P, _P, _P, _P, _P, _P], _INT),
    "mrts_policy_head_packed_words": ([_P, _I32], _I32),
    "mrts_policy_head_pack_dev": ([_P, _I32, _P, _P, _P, _I32, _P, _P], _INT),
    "mrts_policy_head_pack_status": ([_P, _PI64], _INT),
    "mrts_policy_head_unpack_dev": ([_P, _I32, _P, _I32, _I32, _P, _P, _P, _P], _INT),
    "mrts_policy_head_score_packed_dev": ([_P, _I32, _P, _P, _I32, _I32, _P, _P, _P, _P], _INT),
    "mrts_policy_head_grad_packed_dev": ([_P, _I32, _P, _P, _I32, _I32, _P, _P, _P, _P, _P], _INT),
    "mrts_policy_head_sample_typed_dev": ([_P, _I32, _P, _P, _P, _U64, _U32, _P, _P, _P, _P], _INT),
    "mrts_policy_head_score_typed_dev": ([_P, _I32, _I32, _P, _P, _P, _P, _P, _P], _INT),
    "mrts_policy_head_grad_typed_dev": ([_P, _I32, _I32, _P, _P, _P, _P, _P, _P, _P], _INT),
    "mrts_policy_head_score_packed_typed_dev": ([_P, _I32, _I32, _P, _P, _I32, _I32, _P, _P, _P, _P], _INT),
    "mrts_policy_head_grad_packed_typed_dev": ([_P, _I32, _I32, _P, _P, _I32, _I32, _P, _P, _P, _P, _P], _INT),
    "mrts_set_source_output": ([_P, _P], _INT),
    "mrts_onehot_features": ([_P], _INT),
    "mrts_onehot_dev": ([_P, _P, _P, _P], _INT),
    "mrts_obs_packed_words": ([_P, _I32], _I32),
    "mrts_obs_pack_dev": ([_P, _I32, _P, _I32, _P, _P], _INT),
    "mrts_obs_unpack_dev": ([_P, _I32, _P, _I32, _I32, _P, _P, _P], _INT),
    "mrts_obs_onehot_packed_dev": ([_P, _I32, _P, _I32, _I32, _P, _P, _P], _INT),
    "mrts_obs_packed_status": ([_P, _PI64, _PI64], _INT),
    "mrts_copy_games": ([_P, _P, _P, _I32], _INT),
    "mrts_copy_games_dev": ([_P, _P, _P, _I32, _P], _INT),
    "mrts_playout": ([_P, _I32], _INT),
    "mrts_playout_dev": ([_P, _I32, _P], _INT),
    "mrts_evaluate": ([_P, _I32, _P], _INT),
    "mrts_evaluate_dev": ([_P, _I32, _P, _P], _INT),
    "mrts_trace_step": ([_P, _P, _I32, _P, _P, _I32], _INT),
    "mrts_get_state": ([_P, _I32, _P, _I32], _INT),
    "mrts_utt_json": ([_I32, _I32, _C, _C, _I32], _INT),
    "mrts_error_flags": ([_P, _P], _INT),
    "mrts_env_steps": ([_P, _P], _INT),
    "mrts_get_state_json": ([_P, _I32, _C, _I32], _INT),
    "mrts_set_state_json": ([_P, _I32, _C], _INT),
    "mrts_checkpoint_size": ([_P], _I64),
    "mrts_checkpoint": ([_P, _P, _I64], _INT),
    "mrts_restore": ([_P, _P, _I64], _INT),
    "mrts_stream": ([_P], _P),
    "mrts_destroy": ([_P], None),
    "mrts_last_error": ([], _C),
}
EXPORTS = list(SIGNATURES)  # every symbol include/mrts.h declares

_lib = None


def load(path=LIB_PATH):
    """Load libmrts.so; raises ImportError (loudly) when the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise ImportError(f"libmrts.so not found at {path}: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
                          " (no CPU fallback exists)")
    # A process may hold only ONE HIP/HSA runtime.  PyTorch-ROCm bundles its own libamdhip64.so;
    # importing torch first makes libmrts.so bind to that same runtime (its DT_NEEDED soname is
    # already satisfied), which is also what lets torch tensors be passed as device pointers.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(path)
    for name, (argtypes, restype) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = argtypes, restype
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise RuntimeError(f"mrts error {rc}: {load().mrts_last_error().decode()}")
