"""Calls the library refuses before it enqueues a launch, a copy or an allocation, as (name, call) pairs over two
live handles, and what each answers: (return code, mrts_last_error()).  tests/test_gpu_refusals.py compares the
answers with tests/golden/refusals_parent.json, which this module recorded from the library of the commit before
the host runtime got its one entry guard:

    MRTS_LIB_PATH=<that commit's libmrts.so> python -m tests.refusal_cases tests/golden/refusals_parent.json

Every case was read off that commit's mrts_host.cpp: the refusing check precedes the entry point's first
hipMalloc / hipMemcpy / launch (hipSetDevice may precede it).  No case passes a pointer the library would hand to
a kernel: the buffers that are not a case's subject are the handle's own live tensors, and a misaligned pointer is
refused by checkAlign.  Null handles are not here (their text changed with the guard; tests/test_abi_cpu.py)."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M8 = "maps/8x8/basesWorkers8x8.xml"


def _create_refusals(L, _lib):
    """mrts_create on configurations its host-only validation refuses (no device call is reached)"""
    P32 = ctypes.POINTER(ctypes.c_int32)
    good = os.path.join(ROOT, M8).encode()

    def create(n_sp=2, n_bot=0, paths=(good, good), utt_version=1, crs=1, bot=None, ai1=None, n_rewards=0, rewards=None,
               forward_model=0, partial_obs=0, max_units=0, utt_json=None):
        pa = (ctypes.c_char_p * len(paths))(*paths) if paths is not None else None
        bk = (ctypes.c_int32 * len(bot))(*bot) if bot else None
        a1 = (ctypes.c_int32 * len(ai1))(*ai1) if ai1 else None
        rk = (ctypes.c_int32 * len(rewards))(*rewards) if rewards else None
        cfg = _lib.MrtsConfig(n_sp, n_bot, 100, partial_obs, utt_version, crs, ctypes.cast(bk, P32) if bk else None,
                              ctypes.cast(a1, P32) if a1 else None,
                              ctypes.cast(pa, ctypes.POINTER(ctypes.c_char_p)) if pa is not None else None, 0, 0, 0, 0,
                              ctypes.cast(rk, P32) if rk else None, n_rewards, forward_model, utt_json, max_units)
        h = ctypes.c_void_p()
        rc = L.mrts_create(ctypes.byref(cfg), ctypes.byref(h))
        assert rc != 0 and not h.value, "a refusal case created a handle"
        return rc

    return [
        ("create: null arguments", lambda: L.mrts_create(None, None)),
        ("create: odd self-play slots", lambda: create(n_sp=3)),
        ("create: negative bot envs", lambda: create(n_bot=-1)),
        ("create: no environments", lambda: create(n_sp=0)),
        ("create: null map_paths", lambda: create(paths=None)),
        ("create: utt_version 4", lambda: create(utt_version=4)),
        ("create: conflict_policy 0", lambda: create(crs=0)),
        ("create: utt_json that is no JSON", lambda: create(utt_json=b"{broken")),
        ("create: 9 rewards", lambda: create(n_rewards=9)),
        ("create: null reward_kinds", lambda: create(n_rewards=1)),
        ("create: unknown reward function", lambda: create(n_rewards=1, rewards=[8])),
        ("create: ai1_kinds with self-play slots", lambda: create(n_bot=1, paths=(good,) * 3, ai1=[0])),
        ("create: forward model without ai1_kinds", lambda: create(n_sp=0, n_bot=1, paths=(good,), forward_model=1)),
        ("create: forward model with partial_obs", lambda: create(n_sp=0, n_bot=1, paths=(good,), ai1=[0], forward_model=1,
                                                                  partial_obs=1)),
        ("create: unknown bot kind", lambda: create(n_sp=0, n_bot=1, paths=(good,), bot=[3])),
        ("create: LightRush playout policy", lambda: create(n_sp=0, n_bot=1, paths=(good,), ai1=[2], forward_model=1)),
        ("create: LightRush opponent under partial_obs", lambda: create(n_sp=0, n_bot=1, paths=(good,), bot=[2], partial_obs=1)),
        ("create: null map path", lambda: create(paths=(None, None))),
        ("create: missing map file", lambda: create(paths=(b"no/such/map.xml",) * 2)),
        ("create: maps of two sizes", lambda: create(n_sp=4, paths=(good, good, os.path.join(ROOT, "maps/4x4/base4x4.xml").encode(),
                                                                 good))),
        ("create: negative max_units", lambda: create(max_units=-1)),
    ]


def cases(L, _lib, env, fm):
    """env: a DeviceVecEnv of two self-play slots and one PassiveAI bot env on the 8x8 map; fm: a one-game
    forward-model _Handle -> [(name, call)]"""
    torch = env.torch
    h, f = env._h.h, fm.h
    P = ctypes.c_void_p
    a, p, o, r, d, m = (t.data_ptr() for t in (env.actions, env.players, env.obs, env._reward, env._done, env.masks))
    s = env._s(None)
    S = env._h.S
    ring_r = torch.zeros((2, S), dtype=torch.float64, device=env.device)
    ring_d = torch.zeros((2, S), dtype=torch.uint8, device=env.device)
    logits = torch.zeros((S, env._h.H * env._h.W, env._h.K - 1), dtype=torch.float32, device=env.device)
    env._keep = (ring_r, ring_d, logits)
    n_ck = L.mrts_checkpoint_size(h)
    ck = ctypes.create_string_buffer(n_ck)
    _lib.check(L.mrts_checkpoint(h, ck, n_ck))  # a real checkpoint (an ordinary call) for the restore cases
    zeros = ctypes.create_string_buffer(n_ck)
    other = ctypes.create_string_buffer(ck.raw, n_ck)
    other[8] = b"\x02"  # version 2
    pairs = (ctypes.c_int32 * 4)(0, 0, 0, 0)
    pairs_far = (ctypes.c_int32 * 2)(0, 7)
    one = (ctypes.c_int32 * 1)(0)
    rows = (ctypes.c_int32 * 8)(2, 0, 0, 0, 0, 0, 0, 0)

    def ring_too_short():
        _lib.check(L.mrts_set_step_responses(h, P(ring_r.data_ptr()), P(ring_d.data_ptr()), 2))
        try:
            return L.mrts_rollout_fused_dev(h, P(a), P(p), P(o), P(r), P(d), P(m), 0, 7, 0, 3, s)
        finally:
            err = L.mrts_last_error()
            _lib.check(L.mrts_set_step_responses(h, None, None, 0))
            assert L.mrts_last_error() == err

    return _create_refusals(L, _lib) + [
        ("step_dev: null actions", lambda: L.mrts_step_dev(h, None, P(p), P(o), P(r), P(d), P(m), 0, s)),
        ("step_dev: misaligned actions", lambda: L.mrts_step_dev(h, P(a + 2), P(p), P(o), P(r), P(d), P(m), 0, s)),
        ("step_dev: misaligned players", lambda: L.mrts_step_dev(h, P(a), P(p + 1), P(o), P(r), P(d), P(m), 0, s)),
        ("step_dev: misaligned obs", lambda: L.mrts_step_dev(h, P(a), P(p), P(o + 4), P(r), P(d), P(m), 0, s)),
        ("step_dev: misaligned reward", lambda: L.mrts_step_dev(h, P(a), P(p), P(o), P(r + 4), P(d), P(m), 0, s)),
        ("step_dev: misaligned masks", lambda: L.mrts_step_dev(h, P(a), P(p), P(o), P(r), P(d), P(m + 8), 0, s)),
        ("reset_dev: misaligned obs", lambda: L.mrts_reset_dev(h, P(p), P(o + 8), P(r), P(d), P(m), 0, s)),
        ("reset_dev: misaligned masks", lambda: L.mrts_reset_dev(h, P(p), P(o), P(r), P(d), P(m + 1), 0, s)),
        ("step_rows_dev: n_rows < 0", lambda: L.mrts_step_rows_dev(h, P(a), -1, P(p), P(o), P(r), P(d), P(m), 0, s)),
        ("step_rows_dev: null rows", lambda: L.mrts_step_rows_dev(h, None, 1, P(p), P(o), P(r), P(d), P(m), 0, s)),
        ("step_rows: n_rows < 0", lambda: L.mrts_step_rows(h, rows, -1, None, None)),
        ("step_rows: null rows", lambda: L.mrts_step_rows(h, None, 1, None, None)),
        ("step: null actions", lambda: L.mrts_step(h, None, None, None)),
        ("step_fused_dev: null masks", lambda: L.mrts_step_fused_dev(h, P(a), P(p), P(o), P(r), P(d), None, 0, 7, 0, s)),
        ("step_fused_dev: null actions", lambda: L.mrts_step_fused_dev(h, None, P(p), P(o), P(r), P(d), P(m), 0, 7, 0, s)),
        ("step_fused_dev: misaligned obs", lambda: L.mrts_step_fused_dev(h, P(a), P(p), P(o + 4), P(r), P(d), P(m), 0, 7, 0, s)),
        ("step_uniform_dev: null actions", lambda: L.mrts_step_uniform_dev(h, None, P(p), P(o), P(r), P(d), None, 0, 7, 0, s)),
        ("step_uniform_dev: misaligned actions", lambda: L.mrts_step_uniform_dev(h, P(a + 1), P(p), P(o), P(r), P(d), None, 0, 7, 0,
                                                                               s)),
        ("policy_uniform_dev: null actions", lambda: L.mrts_policy_uniform_dev(h, 7, 0, None, s)),
        ("policy_uniform_dev: misaligned actions", lambda: L.mrts_policy_uniform_dev(h, 7, 0, P(a + 2), s)),
        ("rollout_fused_dev: n_steps < 0", lambda: L.mrts_rollout_fused_dev(h, P(a), P(p), P(o), P(r), P(d), P(m), 0, 7, 0, -1, s)),
        ("rollout_fused_dev: null masks", lambda: L.mrts_rollout_fused_dev(h, P(a), P(p), P(o), P(r), P(d), None, 0, 7, 0, 2, s)),
        ("rollout_uniform_dev: n_steps < 0, fused", lambda: L.mrts_rollout_uniform_dev(h, P(a), P(p), P(o), P(r), P(d), 7, 0, -1, 1, s)),
        ("rollout_uniform_dev: n_steps < 0, unfused", lambda: L.mrts_rollout_uniform_dev(h, P(a), P(p), P(o), P(r), P(d), 7, 0, -1, 0,
                                                                                      s)),
        ("rollout_uniform_dev: null actions, fused", lambda: L.mrts_rollout_uniform_dev(h, None, P(p), P(o), P(r), P(d), 7, 0, 2, 1, s)),
        ("rollout_uniform_dev: null actions, unfused", lambda: L.mrts_rollout_uniform_dev(h, None, P(p), P(o), P(r), P(d), 7, 0, 2, 0,
                                                                                       s)),
        ("set_step_responses: one ring", lambda: L.mrts_set_step_responses(h, P(ring_r.data_ptr()), None, 2)),
        ("set_step_responses: max_steps 0", lambda: L.mrts_set_step_responses(h, P(ring_r.data_ptr()), P(ring_d.data_ptr()), 0)),
        ("rollout_fused_dev: a ring shorter than n_steps", ring_too_short),
        ("rollout_fused_records_dev: n_steps < 0", lambda: L.mrts_rollout_fused_records_dev(h, P(a), P(p), P(o), P(r), P(d), P(m), 0, 7,
                                                                                         0, -1, P(o), None, s)),
        ("rollout_fused_records_dev: before exchange_init", lambda: L.mrts_rollout_fused_records_dev(
            h, P(a), P(p), P(o), P(r), P(d), P(m), 0, 7, 0, 2, P(o), None, s)),
        ("rollout_uniform_records_dev: before exchange_init", lambda: L.mrts_rollout_uniform_records_dev(
            h, P(a), P(p), P(o), P(r), P(d), 7, 0, 2, P(o), None, s)),
        ("rollout_fused_exchange_dev: before exchange_init", lambda: L.mrts_rollout_fused_exchange_dev(
            h, P(a), P(p), P(o), P(r), P(d), P(m), 0, 7, 0, 2, P(o), P(o), P(o), s)),
        ("rollout_uniform_exchange_dev: before exchange_init", lambda: L.mrts_rollout_uniform_exchange_dev(
            h, P(a), P(p), P(o), P(r), P(d), 7, 0, 2, P(o), P(o), P(o), s)),
        ("rollout_uniform_exchange_dev: n_steps < 0", lambda: L.mrts_rollout_uniform_exchange_dev(
            h, P(a), P(p), P(o), P(r), P(d), 7, 0, -1, P(o), P(o), P(o), s)),
        ("exchange_init_loopback: no ranks", lambda: L.mrts_exchange_init_loopback(h, 0, 0)),
        ("exchange_init_loopback: rank out of range", lambda: L.mrts_exchange_init_loopback(h, 2, 2)),
        ("exchange_init: null id", lambda: L.mrts_exchange_init(h, None, 1, 0, None)),
        ("set_exchange_bytes: 3", lambda: L.mrts_set_exchange_bytes(h, 3)),
        ("set_obs16: misaligned", lambda: L.mrts_set_obs16(h, P(o + 4))),
        ("set_records: 70000 units", lambda: L.mrts_set_records(h, 70000, 0)),
        ("set_records: negative steps per launch", lambda: L.mrts_set_records(h, 8, -1)),
        ("set_records: a handle with a bot env", lambda: L.mrts_set_records(h, 8, 0)),
        ("render_records_dev: before set_records", lambda: L.mrts_render_records_dev(h, P(o), 64, 1, 0, P(o), 4, s)),
        ("render_records_dev: null records", lambda: L.mrts_render_records_dev(h, None, 64, 1, 0, P(o), 4, s)),
        ("render_records_onehot_dev: before set_records", lambda: L.mrts_render_records_onehot_dev(h, P(o), 64, 1, 0, None, None, 0,
                                                                                                P(o), s)),
        ("get_masks_dev: null out", lambda: L.mrts_get_masks_dev(h, 0, None, s)),
        ("get_masks_dev: misaligned out", lambda: L.mrts_get_masks_dev(h, 0, P(m + 4), s)),
        ("get_masks_i32_dev: null out", lambda: L.mrts_get_masks_i32_dev(h, 0, None, s)),
        ("get_masks: null out", lambda: L.mrts_get_masks(h, 0, None)),
        ("get_masks_i32: null out", lambda: L.mrts_get_masks_i32(h, 0, None)),
        ("get_masks_host: null out", lambda: L.mrts_get_masks_host(h, 0, None)),
        ("get_masks_i32_host: null out", lambda: L.mrts_get_masks_i32_host(h, 0, None)),
        ("onehot_dev: null obs", lambda: L.mrts_onehot_dev(h, None, P(o), s)),
        ("get_state: slot -1", lambda: L.mrts_get_state(h, -1, None, 0)),
        ("get_state: slot past the end", lambda: L.mrts_get_state(h, S, None, 0)),
        ("get_state_json: slot past the end", lambda: L.mrts_get_state_json(h, S, None, 0)),
        ("set_state_json: slot -1", lambda: L.mrts_set_state_json(h, -1, b"{}")),
        ("set_state_json: null text", lambda: L.mrts_set_state_json(h, 0, None)),
        ("checkpoint: null buffer", lambda: L.mrts_checkpoint(h, None, n_ck)),
        ("checkpoint: a buffer one byte short", lambda: L.mrts_checkpoint(h, zeros, n_ck - 1)),
        ("restore: null buffer", lambda: L.mrts_restore(h, None, n_ck)),
        ("restore: too short for a header", lambda: L.mrts_restore(h, ck, 8)),
        ("restore: wrong magic", lambda: L.mrts_restore(h, zeros, n_ck)),
        ("restore: another version", lambda: L.mrts_restore(h, other, n_ck)),
        ("restore: one byte short", lambda: L.mrts_restore(h, ck, n_ck - 1)),
        ("restore: another handle's checkpoint", lambda: L.mrts_restore(f, ck, n_ck)),
        ("capture_begin: the default stream", lambda: L.mrts_capture_begin(h, None)),
        ("capture_end: the default stream", lambda: L.mrts_capture_end(h, None)),
        ("replay: nothing captured", lambda: L.mrts_replay(h, s)),
        ("policy_head_score_dev: n_rows < 0", lambda: L.mrts_policy_head_score_dev(h, -1, P(logits.data_ptr()), P(m), P(a), None, None,
                                                                                 s)),
        ("policy_head_score_dev: null logits", lambda: L.mrts_policy_head_score_dev(h, S, None, P(m), P(a), None, None, s)),
        ("policy_head_sample_dev: misaligned logprob", lambda: L.mrts_policy_head_sample_dev(h, P(logits.data_ptr()), P(m), None, 7, 0,
                                                                                           P(a), P(o + 2), None, s)),
        ("policy_head_grad_dev: null gradient", lambda: L.mrts_policy_head_grad_dev(h, S, P(logits.data_ptr()), P(m), P(a), None, None,
                                                                                  None, s)),
        ("policy_head_packed_words: cap 0", lambda: L.mrts_policy_head_packed_words(h, 0)),
        ("policy_head_pack_dev: cap past H*W", lambda: L.mrts_policy_head_pack_dev(h, S, P(m), None, P(a), 65, P(o), s)),
        ("policy_head_pack_dev: null packed", lambda: L.mrts_policy_head_pack_dev(h, S, P(m), None, P(a), 8, None, s)),
        ("policy_head_pack_status: null out", lambda: L.mrts_policy_head_pack_status(h, None)),
        ("policy_head_unpack_dev: no packed rows", lambda: L.mrts_policy_head_unpack_dev(h, S, P(o), 0, 8, None, P(m), P(a), s)),
        ("policy_head_score_packed_dev: null logits", lambda: L.mrts_policy_head_score_packed_dev(h, S, None, P(o), S, 8, None, None,
                                                                                               None, s)),
        ("policy_head_grad_packed_dev: null packed", lambda: L.mrts_policy_head_grad_packed_dev(h, S, P(logits.data_ptr()), None, S, 8,
                                                                                             None, None, None, P(logits.data_ptr()),
                                                                                             s)),
        ("evaluate_dev: null out", lambda: L.mrts_evaluate_dev(h, 0, None, s)),
        ("evaluate_dev: maxplayer 2", lambda: L.mrts_evaluate_dev(h, 2, P(r), s)),
        ("evaluate: null out", lambda: L.mrts_evaluate(h, 0, None)),
        ("playout_dev: not a forward model", lambda: L.mrts_playout_dev(h, 10, s)),
        ("playout: not a forward model", lambda: L.mrts_playout(h, 10)),
        ("trace_step: not a forward model", lambda: L.mrts_trace_step(h, None, 0, one, None, 0)),
        ("copy_games: destination is no forward model", lambda: L.mrts_copy_games(h, None, pairs, 1)),
        ("copy_games_dev: destination is no forward model", lambda: L.mrts_copy_games_dev(h, None, P(p), 1, s)),
        # the forward-model handle
        ("forward model: step_dev", lambda: L.mrts_step_dev(f, P(a), P(p), P(o), P(r), P(d), None, 0, s)),
        ("forward model: step_rows_dev", lambda: L.mrts_step_rows_dev(f, P(a), 1, P(p), P(o), P(r), P(d), None, 0, s)),
        ("forward model: step_fused_dev", lambda: L.mrts_step_fused_dev(f, P(a), P(p), P(o), P(r), P(d), P(m), 0, 7, 0, s)),
        ("forward model: step_uniform_dev", lambda: L.mrts_step_uniform_dev(f, P(a), P(p), P(o), P(r), P(d), None, 0, 7, 0, s)),
        ("forward model: rollout_fused_dev", lambda: L.mrts_rollout_fused_dev(f, P(a), P(p), P(o), P(r), P(d), P(m), 0, 7, 0, 2, s)),
        ("forward model: rollout_uniform_dev", lambda: L.mrts_rollout_uniform_dev(f, P(a), P(p), P(o), P(r), P(d), 7, 0, 2, 1, s)),
        ("forward model: policy_head_score_dev", lambda: L.mrts_policy_head_score_dev(f, 1, P(logits.data_ptr()), P(m), P(a), None,
                                                                                    None, s)),
        ("forward model: policy_head_packed_words", lambda: L.mrts_policy_head_packed_words(f, 8)),
        ("forward model: policy_head_pack_dev", lambda: L.mrts_policy_head_pack_dev(f, 1, P(m), None, P(a), 8, P(o), s)),
        ("forward model: playout_dev horizon past the bound", lambda: L.mrts_playout_dev(f, _lib.MRTS_MAX_HORIZON + 1, s)),
        ("forward model: playout horizon below the bound", lambda: L.mrts_playout(f, -_lib.MRTS_MAX_HORIZON - 1)),
        ("forward model: trace_step null until", lambda: L.mrts_trace_step(f, None, 0, None, None, 0)),
        ("forward model: trace_step n_pairs < 0", lambda: L.mrts_trace_step(f, rows, -1, one, None, 0)),
        ("forward model: trace_step null pairs", lambda: L.mrts_trace_step(f, None, 1, one, None, 0)),
        ("forward model: trace_step pair player 2", lambda: L.mrts_trace_step(f, rows, 1, one, None, 0)),
        ("forward model: copy_games n < 0", lambda: L.mrts_copy_games(f, None, pairs, -1)),
        ("forward model: copy_games null pairs", lambda: L.mrts_copy_games(f, None, None, 1)),
        ("forward model: copy_games game out of range", lambda: L.mrts_copy_games(f, None, pairs_far, 1)),
        ("forward model: copy_games a game onto itself", lambda: L.mrts_copy_games(f, None, pairs, 1)),
        ("forward model: copy_games a destination twice", lambda: L.mrts_copy_games(f, h, pairs, 2)),
        ("forward model: copy_games_dev n < 0", lambda: L.mrts_copy_games_dev(f, None, P(p), -1, s)),
        ("forward model: copy_games_dev null pairs", lambda: L.mrts_copy_games_dev(f, None, None, 1, s)),
        ("forward model: set_records", lambda: L.mrts_set_records(f, 8, 0)),
        ("forward model: get_state slot 1", lambda: L.mrts_get_state(f, 1, None, 0)),
    ]


def handles():
    """-> (L, _lib, env, fm) as cases() wants them"""
    from microrts_amd import DeviceVecEnv, UnitTypeTable, _lib
    from microrts_amd.vec_client import _Handle

    env = DeviceVecEnv(2, 1, 2000, [M8] * 3, ai2s=["PassiveAI"], seed=11)
    fm = _Handle(0, 1, 2000, [os.path.join(ROOT, M8)], ["PassiveAI"], UnitTypeTable(), False, 0, 11, 0, ai1s=["PassiveAI"],
                 forward_model=True)
    return _lib.load(), _lib, env, fm


def answers(L, _lib, env, fm):
    """-> [[name, return code, mrts_last_error()]] in table order; every case must be a refusal"""
    out = []
    for name, call in cases(L, _lib, env, fm):
        rc = call()
        assert rc < 0, f"{name}: not refused ({rc})"
        out.append([name, rc, L.mrts_last_error().decode()])
    assert len({n for n, _, _ in out}) == len(out), "case names repeat"
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    L, lib_mod, env, fm = handles()
    table = answers(L, lib_mod, env, fm)
    env.close()
    fm.close()
    with open(sys.argv[1], "w") as fh:
        json.dump(table, fh, indent=0)
        fh.write("\n")
    print(f"{len(table)} refusals recorded from {lib_mod.LIB_PATH}")
