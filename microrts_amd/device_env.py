"""DeviceVecEnv: the zero-copy rollout form of the env over the libmrts C ABI — every buffer is a torch tensor in HBM
and all calls are ordered on torch's current HIP stream (no host sync).  There is no CPU fallback: constructing it
without a GPU or without libmrts.so raises."""
import ctypes
import operator

import numpy as np

from . import _lib, obs_pack, policy_head
from ._device import DeviceHandle
from ._packed import check_tensor
from .vec_client import UnitTypeTable, _check_rfs, _Handle, _resolve


class DeviceVecEnv(DeviceHandle):
    """Zero-copy rollout backend: torch HBM tensors; every call is ordered on torch's CURRENT HIP
    stream of the env's device (or an explicit `stream=`), so ordinary torch ops on the tensors need
    no extra synchronisation."""

    def __init__(self, num_selfplay_slots, num_bot_envs, max_steps, map_paths, ai2s=None, utt=None, partial_obs=False,
                 device=0, seed=0, slot_id_base=0, with_masks=True, ai1s=None, mask_delta=True, source_bits=True,
                 rfs=None, max_units=0, obs_delta=True):
        """ai2s / ai1s: the bot of each bot env (names or objects named like the Java classes); a missing
        or short list is padded with PassiveAI (the JNIGridnetVecClient mirror raises instead, like
        Java).  mask_delta: `masks` is owned by this object and reused every call, so only changed rows are
        rewritten (the tensor must not be written by the caller).  source_bits: also keep mask slot 0
        as bits in `source` ([slots][ceil(H*W/32)] int32), which random_policy uses.  rfs: reward
        function names (a_rfs); reward / done are [S] for one function, [S][R] otherwise.  obs_delta:
        `obs` is persistent too (mrts_set_obs_delta: partially observable views re-render only the chunks
        that can have changed); an in-place torch write to `obs` (its version counter moves) makes the
        next write a full one."""
        torch = self._open("DeviceVecEnv", device)
        utt = utt or UnitTypeTable()
        paths = [_resolve("", p) for p in map_paths]
        self._h = _Handle(num_selfplay_slots, num_bot_envs, max_steps, paths, ai2s, utt, partial_obs, device, seed,
                          slot_id_base, ai1s=ai1s, mask_delta=mask_delta and with_masks, rewards=_check_rfs(rfs),
                          max_units=max_units)
        h = self._h
        self.mask_delta = bool(mask_delta and with_masks)
        dev = self.device
        S, H, W, C, K = h.S, h.H, h.W, h.C, h.K
        self.obs = torch.zeros((S, C, H, W), dtype=torch.int32, device=dev)
        rshape = (S,) if h.R == 1 else (S, h.R)
        self._reward = torch.zeros(rshape, dtype=torch.float64, device=dev)
        self._done = torch.zeros(rshape, dtype=torch.uint8, device=dev)
        self._ring_last = None  # ring step holding the last rollout call's responses (set_step_responses)
        self.masks = torch.zeros((S, H, W, K), dtype=torch.uint8, device=dev) if with_masks else None
        self.actions = torch.zeros((S, H * W, 7), dtype=torch.int32, device=dev)
        self.players = torch.zeros((S,), dtype=torch.int32, device=dev)
        self.source = torch.zeros((S, (H * W + 31) // 32), dtype=torch.int32, device=dev) if (with_masks and source_bits) else None
        if self.source is not None:
            _lib.check(h.L.mrts_set_source_output(h.h, self._p(self.source)))
        self.mask_player = 0
        self.partial_obs = bool(partial_obs)
        self.step_rewards = self.step_dones = None
        self._policy_out, self._policy_version = None, -1
        _lib.check(h.L.mrts_set_obs_delta(h.h, int(bool(obs_delta))))
        self._obs_version = -1
        self._ptr_cache = None
        torch.cuda.synchronize(dev)

    @property
    def reward(self):
        """The last step's reward ([slots] or [slots][R], float64).  After a rollout call that wrote the Responses
        ring (set_step_responses), this is the ring's last step of that call (a view: no copy), else
        the plain buffer the step calls write."""
        return self._reward if self._ring_last is None else self.step_rewards[self._ring_last]

    @property
    def done(self):
        """The last step's done flags (uint8, as reward; the ring's last step after a ring-writing rollout)."""
        return self._done if self._ring_last is None else self.step_dones[self._ring_last]

    def _bufs(self):
        """actions, players, obs, reward, done, masks as ctypes pointers, cached while the same tensor
        objects stay attached (the rollout calls' per-call host cost)."""
        key = (self.actions, self.players, self.obs, self._reward, self._done, self.masks)
        c = self._ptr_cache
        if c is None or not all(map(operator.is_, c[0], key)):
            c = self._ptr_cache = (key, tuple(self._p(t) for t in key))
        return c[1]

    def set_rollout_events(self, start, end):
        """The next rollout_fused / rollout_uniform call records these hipEvent_t handles (ints or
        ctypes pointers, None = skip) right before its first and after its last kernel launch
        (mrts_set_rollout_events): a benchmark's events bracket exactly the rollout's kernels."""
        _lib.check(self._h.L.mrts_set_rollout_events(self._h.h, start, end))

    def _policy_stale(self, out):
        """`out` is the tensor holding the library's last policy output, and someone else wrote it since."""
        return self._policy_out is out and out._version != self._policy_version

    def _policy_stamp(self, out):
        """`out` holds the library's policy output as of now; None: no tensor does."""
        self._policy_out, self._policy_version = out, -1 if out is None else out._version

    def _write(self, entry, tail, stream, n_steps=None, policy=False, masks=True, lead=None):
        """The bracket around every entry point that writes `obs`: the guards, the call
        h.L.<entry>(handle, *lead, players, obs, reward, done, [masks, mask_player,] *tail, stream) on the cached
        pointers, then the bookkeeping, none of which runs if the call raises.  lead: what stands before players
        (default: the actions).  masks: True, False (a null pointer in their place: this call writes none) or None
        (the entry takes no masks).  n_steps: a rollout of that many steps (with the Responses ring on, its responses
        are in ring steps 0 .. n_steps - 1); None: a single step (it writes the plain reward / done).  policy: the
        entry decodes and then resamples env.actions (the fused policy)."""
        h = self._h
        if policy and self._policy_stale(self.actions):
            _lib.check(h.L.mrts_policy_invalidate(h.h))  # written by someone else since
        if self.obs._version != self._obs_version:  # a torch in-place write since our last one voids the delta base
            _lib.check(h.L.mrts_obs_invalidate(h.h))
        a, pl, o, r, d, m = self._bufs()
        mk = () if masks is None else (m if masks else None, self.mask_player)
        rc = getattr(h.L, entry)(h.h, *((a,) if lead is None else lead), pl, o, r, d, *mk, *tail, self._s(stream))
        if rc:  # (no call on the way out of a step that went well: this is the rollout loop's host cost)
            _lib.check(rc)
        if n_steps is None:
            self._ring_last = None
        elif self.step_rewards is not None and n_steps > 0:
            self._ring_last = n_steps - 1
        self._obs_version = self.obs._version
        if policy:
            self._policy_stamp(self.actions)

    def reset(self, stream=None):
        self._write("mrts_reset_dev", (), stream, lead=())

    def step(self, actions=None, stream=None, masks=True):
        """masks=False: this step writes no masks (the masks tensor keeps its previous contents)."""
        self._write("mrts_step_dev", (), stream, masks=bool(masks), lead=None if actions is None else (self._p(actions),))

    def uniform_policy(self, seed, step, out=None, stream=None):
        """Unmasked uniform random rows for every cell (BASELINE config c2; mrts_policy_uniform_dev):
        type in [0,6), directions in [0,4), produce type in [0,ntypes), attack index in [0,K-23-ntypes)."""
        h = self._h
        out = self.actions if out is None else out
        _lib.check(h.L.mrts_policy_uniform_dev(h.h, seed, step, self._p(out), self._s(stream)))
        return out

    def step_uniform(self, seed, step, masks=False, stream=None):
        """uniform_policy(seed, step) into env.actions, then step() on it — in one launch
        (mrts_step_uniform_dev: the step kernel writes the rows and draws its idle units' rows itself)."""
        self._write("mrts_step_uniform_dev", (seed, step), stream, masks=bool(masks))

    def rollout_uniform(self, seed, first_step, n_steps, fused=True, stream=None):
        """n_steps x (uniform_policy(seed, first_step + k), then a step without masks), enqueued by
        native code (mrts_rollout_uniform_dev): the c2 random-policy rollout.  fused: one
        step_uniform launch per step (same results) instead of a policy launch + a step launch."""
        self._write("mrts_rollout_uniform_dev", (seed, first_step, n_steps, 1 if fused else 0), stream, n_steps, masks=None)

    def step_fused(self, seed, next_step, stream=None):
        """step() on env.actions, then env.actions := random_policy(seed, next_step) from the masks this
        step wrote (mrts_step_fused_dev: one launch, identical result)."""
        assert self.masks is not None, "the fused policy samples from the masks"
        self._write("mrts_step_fused_dev", (seed, next_step), stream, policy=True)

    def set_obs16(self, out):
        """Every later observation write also fills `out` (int16 [n_slots][C][H][W], or None = off) —
        the observation exchange's compact transport, written by the step kernel
        (mrts_set_obs16; full observability)."""
        import torch
        if out is not None:
            assert out.dtype == torch.int16 and tuple(out.shape) == tuple(self.obs.shape) and out.is_contiguous()
        _lib.check(self._h.L.mrts_set_obs16(self._h.h, self._p(out) if out is not None else None))
        self._obs16 = out  # keep it alive while the handle writes into it

    def set_multi_step(self, on):
        """rollout_fused may run several steps per launch (default; mrts_set_multi_step)."""
        _lib.check(self._h.L.mrts_set_multi_step(self._h.h, 1 if on else 0))

    @property
    def multi_step_capable(self):
        """The handle's shape and switch allow multi-step launches (mrts_multi_step_capable):
        rollout_uniform uses them; rollout_fused only with mask_delta (see fused_multi_step)."""
        return bool(self._h.L.mrts_multi_step_capable(self._h.h))

    @property
    def fused_multi_step(self):
        """rollout_fused runs several steps per launch on this handle: the shape allows it and the
        handle keeps delta masks (the steady fused state needs them)."""
        return self.multi_step_capable and bool(self.mask_delta)

    def rollout_fused(self, seed, first_next_step, n_steps, stream=None):
        """n_steps step_fused calls (next_step = first_next_step, first_next_step + 1, ...) enqueued by
        native code (mrts_rollout_fused_dev): no Python between them; on the specialised
        full-observability self-play shapes, in the steady fused state, up to MRTS_MAX_ITER steps per
        launch (each game's state kept in LDS between its steps) — bit-identical results."""
        assert self.masks is not None, "the fused policy samples from the masks"
        self._write("mrts_rollout_fused_dev", (seed, first_next_step, n_steps), stream, n_steps, policy=True)

    def rollout_fused_exchange(self, seed, first_next_step, n_steps, send, recv, stream=None):
        """rollout_fused with one launch per step and the all-gather of every step's int16 observation
        into recv (mrts_rollout_fused_exchange_dev; microrts_amd.dist.NativeExchange sets it up)."""
        self._write("mrts_rollout_fused_exchange_dev",
                    (seed, first_next_step, n_steps, self._p(send[0]), self._p(send[1]), self._p(recv)), stream, n_steps,
                    policy=True)

    def capture(self, fn, stream):
        """Capture the calls fn() makes on this handle on `stream` (a non-default torch stream, made
        current during fn) as one graph (mrts_capture_begin / _end); replay() launches it."""
        h = self._h
        s = ctypes.c_void_p(stream.cuda_stream)
        with self.torch.cuda.stream(stream):
            _lib.check(h.L.mrts_capture_begin(h.h, s))
            try:
                fn()
            finally:
                _lib.check(h.L.mrts_capture_end(h.h, s))

    def replay(self, stream=None):
        """Launch the graph capture() built (the same calls, verbatim) on `stream` (default: current)."""
        _lib.check(self._h.L.mrts_replay(self._h.h, self._s(stream)))

    def rollout_uniform_exchange(self, seed, first_step, n_steps, send, recv, stream=None):
        """rollout_uniform (fused form) with the all-gather of every step's int16 observation
        (mrts_rollout_uniform_exchange_dev)."""
        self._write("mrts_rollout_uniform_exchange_dev",
                    (seed, first_step, n_steps, self._p(send[0]), self._p(send[1]), self._p(recv)), stream, n_steps,
                    masks=None)

    def set_records(self, units_per_record=64, steps_per_launch=0):
        """Enable the compact observation records (mrts_set_records): units per game record (0 = off) and
        steps per launch of a records rollout (0 = as many as a launch runs).  Returns words per record."""
        _lib.check(self._h.L.mrts_set_records(self._h.h, int(units_per_record), int(steps_per_launch)))
        self.record_units = int(units_per_record)
        self.record_words = int(self._h.L.mrts_record_words(self._h.h))
        return self.record_words

    def records_buffer(self, n_steps, world=1):
        """A receive buffer for n_steps of a records rollout over `world` ranks (uint32 words)."""
        return self.torch.zeros(n_steps * world * (self._h.S // 2) * self.record_words, dtype=self.torch.int32,
                                device=self.device)

    def rollout_fused_records(self, seed, first_next_step, n_steps, recv, stream=None):
        """rollout_fused whose every step's game records are all-gathered into recv
        (mrts_rollout_fused_records_dev; microrts_amd.dist.RecordExchange sets it up).  Returns the
        per-step (word offset of rank 0's records, rank stride) as int64 [n_steps, 2]."""
        off = np.zeros((max(n_steps, 1), 2), dtype=np.int64)
        self._write("mrts_rollout_fused_records_dev", (seed, first_next_step, n_steps, self._p(recv), off.ctypes.data), stream,
                    n_steps, policy=True)
        return off[:n_steps]

    def rollout_uniform_records(self, seed, first_step, n_steps, recv, stream=None):
        """rollout_uniform (fused form) whose every step's game records are all-gathered into recv
        (mrts_rollout_uniform_records_dev).  Returns the per-step offsets as rollout_fused_records."""
        off = np.zeros((max(n_steps, 1), 2), dtype=np.int64)
        self._write("mrts_rollout_uniform_records_dev", (seed, first_step, n_steps, self._p(recv), off.ctypes.data), stream,
                    n_steps, masks=None)
        return off[:n_steps]

    def render_records(self, recv, offset, rank_stride, n_ranks, out, stream=None):
        """The observations of n_ranks x games records (rank r's at recv[offset + r * rank_stride:]) into
        out [n_ranks * slots, C, H, W] (uint8 or int32; int8 or int32 for a partially observable handle) —
        mrts_render_records_dev."""
        h = self._h
        ob = out.element_size()
        T = self.torch
        # a partially observable view shows a dead unit's hp (<= 0): int8, never uint8
        ok = (T.int8, T.int32) if self.partial_obs else (T.uint8, T.int32)
        assert out.dtype in ok, f"render_records: out must be one of {ok}, not {out.dtype}"
        assert out.is_contiguous() and out.numel() == n_ranks * self.obs.numel()
        assert recv.dtype == T.int32 and recv.is_contiguous() and 0 <= int(offset) <= recv.numel()
        ptr = ctypes.c_void_p(recv.data_ptr() + 4 * int(offset))
        _lib.check(h.L.mrts_render_records_dev(h.h, ptr, recv.numel() - int(offset), int(n_ranks), int(rank_stride), self._p(out),
                                               ob, self._s(stream)))
        return out

    def render_records_onehot(self, recv, offset, rank_stride, sel, out=None, step_off=None, stream=None, n_ranks=None):
        """A learner minibatch from records in one launch: the MicroRTS-Py one-hot observations (onehot_obs'
        layout, uint8 [n][H][W][F]) of the slots sel (int32 tensor of global indices r * slots + slot over the
        ranks in recv) of the step whose records start at recv[offset] with rank_stride — or, with step_off
        (int64 tensor [n, 2]: each sample's step's row of the rollout's offsets table), each sample's own
        step — mrts_render_records_onehot_dev.  n_ranks (default: as many as recv holds) bounds sel; a sample
        outside recv or n_ranks renders as zeros and raises render_overflow()."""
        h, T = self._h, self.torch
        F = h.L.mrts_onehot_features(h.h)
        assert sel.dtype == T.int32 and sel.is_contiguous() and sel.device == self.device
        if step_off is not None:
            assert step_off.dtype == T.int64 and step_off.is_contiguous() and step_off.numel() == 2 * sel.numel()
        if out is None:
            out = T.empty((sel.numel(), h.H, h.W, F), dtype=T.uint8, device=self.device)
        assert out.dtype == T.uint8 and out.is_contiguous() and out.numel() == sel.numel() * h.H * h.W * F
        assert recv.dtype == T.int32 and recv.is_contiguous() and 0 <= int(offset) <= recv.numel()
        if n_ranks is None:  # every rank place a records buffer of this handle's games can hold
            n_ranks = max(1, recv.numel() // max(1, (h.S // 2) * self.record_words))
        ptr = ctypes.c_void_p(recv.data_ptr() + 4 * int(offset))
        _lib.check(h.L.mrts_render_records_onehot_dev(h.h, ptr, recv.numel() - int(offset), int(n_ranks), int(rank_stride),
                                                      self._p(sel), self._p(step_off), int(sel.numel()), self._p(out),
                                                      self._s(stream)))
        return out

    def render_overflow(self):
        """True if a record rendered since the last call had its overflow bit set (units missing from the
        rendered observation; the sender flagged MRTS_ERR_RECORD) — mrts_render_status, synchronises."""
        r = self._h.L.mrts_render_status(self._h.h)
        if r < 0:
            _lib.check(r)
        return bool(r)

    def set_step_responses(self, max_steps):
        """Every step's reward / done from each rollout call of at most max_steps steps
        (mrts_set_step_responses; Java's gameStep returns them on every call): step k of the next call
        lands in self.step_rewards[k] / self.step_dones[k] ([slots] or [slots][R], as reward / done) INSTEAD
        of the plain reward / done buffers, which rollout calls then leave untouched; after such a call
        self.reward / self.done are views of its last ring step (step_rewards[n_steps - 1]), so they never
        read stale.  0 turns it off."""
        h, T = self._h, self.torch
        if not max_steps:
            _lib.check(h.L.mrts_set_step_responses(h.h, None, None, 0))
            self.step_rewards = self.step_dones = None
            self._ring_last = None
            return
        self._ring_last = None
        self.step_rewards = T.zeros((max_steps,) + tuple(self._reward.shape), dtype=T.float64, device=self.device)
        self.step_dones = T.zeros((max_steps,) + tuple(self._done.shape), dtype=T.uint8, device=self.device)
        _lib.check(h.L.mrts_set_step_responses(h.h, self._p(self.step_rewards), self._p(self.step_dones), int(max_steps)))

    def step_rows(self, rows, stream=None):
        """gameStep with Java rows: int32 [slots][n_rows][8] on this device (any order, duplicates ok)."""
        h = self._h
        assert rows.dtype == self.torch.int32 and rows.is_contiguous() and rows.dim() == 3 and rows.shape[2] == 8
        assert rows.shape[0] == h.S and rows.device == self.device
        self._write("mrts_step_rows_dev", (), stream, lead=(self._p(rows), rows.shape[1]))

    def onehot_obs(self, obs=None, out=None, stream=None):
        """MicroRTS-Py's encoding of the observation (gym_microrts `_encode_obs`: clip + one-hot,
        channels last): uint8 [slots][H][W][F], F = 29 (33 with partial observability)."""
        h = self._h
        F = h.L.mrts_onehot_features(h.h)
        src = self.obs if obs is None else obs
        if out is None:
            out = self.torch.empty((h.S, h.H, h.W, F), dtype=self.torch.uint8, device=self.device)
        _lib.check(h.L.mrts_onehot_dev(h.h, self._p(src), self._p(out), self._s(stream)))
        return out

    def get_masks(self, out=None, stream=None):
        h = self._h
        out = self.masks if out is None else out
        _lib.check(h.L.mrts_get_masks_dev(h.h, self.mask_player, self._p(out), self._s(stream)))
        return out

    def random_policy(self, seed, step, masks=None, out=None, stream=None):
        h = self._h
        m = self.masks if masks is None else masks
        out = self.actions if out is None else out
        src = self.source if masks is None else None
        # the library rewrites only changed rows when `out` still holds its previous output; an
        # in-place write by anyone else bumps the tensor's version counter -> full rewrite
        if self._policy_out is not out or self._policy_stale(out):
            _lib.check(h.L.mrts_policy_invalidate(h.h))
        _lib.check(h.L.mrts_policy_dev(h.h, self._p(m), self._p(src), seed, step, self._p(out), self._s(stream)))
        self._policy_stamp(out)
        return out

    def sample_actions(self, logits, seed, step, out=None, stream=None):
        """The masked policy head (mrts_policy_head_sample_dev; policy_head.py): action rows drawn from `logits`
        (float32, bfloat16 or float16 [slots][H*W][K-1]; 16-bit logits draw what `logits.float()` draws) under env.masks, the candidate cells taken from env.source when it exists.
        Returns (actions, logprob, entropy): `out` (default env.actions, every row written) and float32 [slots]
        sums over each slot's candidate cells.  Philox counters (slot id, step, cell): the same seed, step and
        logits give the same rows."""
        h, T = self._h, self.torch
        if self.masks is None:
            raise ValueError("sample_actions needs the masks (with_masks=True)")
        out = self.actions if out is None else out
        policy_head.check_head_args(self, logits, self.masks, out, n=h.S, actions_name="out")
        logprob = T.empty(h.S, dtype=T.float32, device=self.device)
        entropy = T.empty(h.S, dtype=T.float32, device=self.device)
        lt = policy_head.logits_type(logits)
        if lt == _lib.MRTS_LOGITS_F32:
            _lib.check(h.L.mrts_policy_head_sample_dev(h.h, self._p(logits), self._p(self.masks), self._p(self.source), seed,
                                                       step, self._p(out), self._p(logprob), self._p(entropy), self._s(stream)))
        else:
            _lib.check(h.L.mrts_policy_head_sample_typed_dev(h.h, lt, self._p(logits), self._p(self.masks), self._p(self.source),
                                                             seed, step, self._p(out), self._p(logprob), self._p(entropy),
                                                             self._s(stream)))
        # the library dropped its delta bases (as mrts_policy_invalidate): no tensor holds a tracked policy output
        self._policy_stamp(None)
        return out, logprob, entropy

    def packed_words(self, cap=None):
        """uint32 words of a packed row (policy_head.py; include/mrts.h "Packed policy rows") of at most `cap`
        candidate cells: 1 + cap * 5.  cap: 1 .. H*W, default min(H*W, 64); H*W can never overflow."""
        return policy_head.packed_words(self, cap)

    def packed_buffer(self, n_steps, cap=None):
        """A rollout's masks and action rows, packed: uint32 zeros [n_steps][slots][packed_words(cap)] —
        pack_step(buf[t]) fills step t, evaluate_actions_packed(env, logits, buf, index=mb) scores a minibatch."""
        T = self.torch
        return T.zeros((n_steps, self._h.S, self.packed_words(cap)), dtype=T.int32, device=self.device).view(T.uint32)

    def pack_step(self, out, masks=None, actions=None, cap=None, stream=None):
        """Packs the step's masks and action rows into `out` (uint32 [slots][words], such as buf[t]; every word
        written): one launch (mrts_policy_head_pack_dev).  Default env.masks / env.actions, the candidate cells from
        env.source; with `masks` given, [n][H][W][K] and `actions` [n][H*W][7] for any n = out's rows, the
        candidates come from mask slot 0.  cap defaults to what out's words stand for.  A row of more than cap
        candidates keeps its first cap and is counted (pack_overflow); its score is NaN."""
        h = self._h
        if masks is None and self.masks is None:
            raise ValueError("masks: pack_step needs the masks (with_masks=True)")
        m = self.masks if masks is None else masks
        a = self.actions if actions is None else actions
        src = self.source if masks is None else None
        n, cap = policy_head.check_pack_args(self, out, m, a, src, cap)
        _lib.check(h.L.mrts_policy_head_pack_dev(h.h, n, self._p(m), self._p(src), self._p(a), cap, self._p(out), self._s(stream)))
        return out

    def pack_overflow(self):
        """The rows that pack_step cut at their cap since the last call of this (mrts_policy_head_pack_status);
        clears the count.  Synchronises."""
        v = ctypes.c_int64(0)
        _lib.check(self._h.L.mrts_policy_head_pack_status(self._h.h, ctypes.byref(v)))
        return v.value

    def unpack(self, packed, index=None, masks_out=None, actions_out=None, stream=None):
        """The canonical dense form of packed rows (mrts_policy_head_unpack_dev): (masks uint8 [rows][H][W][K] of
        0 / 1, actions int32 [rows][H*W][7]) with components that were off their field -1 and zeros at
        non-candidate cells.  rows: index's length (int32, gathers packed rows), else every packed row."""
        h, T = self._h, self.torch
        rows, n_packed, cap = policy_head.LAYOUT.check_read(self, packed, index)
        if masks_out is None:
            masks_out = T.empty((rows, h.H, h.W, h.K), dtype=T.uint8, device=self.device)
        if actions_out is None:
            actions_out = T.empty((rows, h.H * h.W, 7), dtype=T.int32, device=self.device)
        check_tensor("masks_out", masks_out, T.uint8, [(rows, h.H, h.W, h.K), (rows, h.H * h.W, h.K)], self.device)
        check_tensor("actions_out", actions_out, T.int32, [(rows, h.H * h.W, 7)], self.device)
        _lib.check(h.L.mrts_policy_head_unpack_dev(h.h, rows, self._p(packed), n_packed, cap, self._p(index),
                                                   self._p(masks_out), self._p(actions_out), self._s(stream)))
        return masks_out, actions_out

    def obs_packed_words(self, cap=None):
        """uint32 words of a packed observation row (obs_pack.py; include/mrts.h "Packed observation rows") of at
        most `cap` occupied cells: 1 + 2 * cap + (C - 5) * ceil(H*W / 32).  cap: 1 .. H*W, default min(H*W, 128);
        H*W can never cut a row."""
        return obs_pack.packed_words(self, cap)

    def obs_packed_buffer(self, n_steps, cap=None):
        """A rollout's observations, packed: uint32 zeros [n_steps][slots][obs_packed_words(cap)] — pack_obs(buf[t])
        fills step t, onehot_packed(buf, index=mb) gives a minibatch's network input."""
        T = self.torch
        return T.zeros((n_steps, self._h.S, self.obs_packed_words(cap)), dtype=T.int32, device=self.device).view(T.uint32)

    def pack_obs(self, out, obs=None, cap=None, stream=None):
        """Packs observations into `out` (uint32 [n][words], such as buf[t]; every word written): one launch
        (mrts_obs_pack_dev).  obs: default env.obs, or any int32 [n][C][H][W] with n = out's rows.  cap defaults to
        what out's words stand for.  A row of more than cap occupied cells keeps its first cap, its true count and
        the lossy flag, and is counted (obs_pack_status)."""
        h = self._h
        src = self.obs if obs is None else obs
        n, cap = obs_pack.check_pack_args(self, out, src, cap)
        _lib.check(h.L.mrts_obs_pack_dev(h.h, n, self._p(src), cap, self._p(out), self._s(stream)))
        return out

    def unpack_obs(self, packed, index=None, out=None, stream=None):
        """The int32 planes [rows][C][H][W] of packed observation rows (mrts_obs_unpack_dev): for a row without the
        lossy flag the tensor that was packed.  packed: uint32 [N][words] or any leading shape (a [T][slots][words]
        rollout buffer), flattened; rows: index's length (int32 on the device, gathers packed rows, repeats allowed),
        else every packed row.  An index outside [0, N) gives a zero row and is counted (obs_pack_status)."""
        h, T = self._h, self.torch
        rows, n_packed, cap = obs_pack.check_read_args(self, packed, index)
        if out is None:
            out = T.empty((rows, h.C, h.H, h.W), dtype=T.int32, device=self.device)
        check_tensor("out", out, T.int32, [(rows, h.C, h.H, h.W)], self.device)
        _lib.check(h.L.mrts_obs_unpack_dev(h.h, rows, self._p(packed), n_packed, cap, self._p(index), self._p(out),
                                           self._s(stream)))
        return out

    def onehot_packed(self, packed, index=None, out=None, stream=None):
        """onehot_obs straight from packed observation rows (mrts_obs_onehot_packed_dev): uint8 [rows][H][W][F], for
        every row that was not cut at its cap the bytes onehot_obs gives on the tensor that was packed.  packed, index
        and rows as unpack_obs: onehot_packed(buf, index=mb) is an update's minibatch, with no dense copy of the
        buffer."""
        h, T = self._h, self.torch
        rows, n_packed, cap = obs_pack.check_read_args(self, packed, index)
        F = h.L.mrts_onehot_features(h.h)
        if out is None:
            out = T.empty((rows, h.H, h.W, F), dtype=T.uint8, device=self.device)
        check_tensor("out", out, T.uint8, [(rows, h.H, h.W, F)], self.device)
        _lib.check(h.L.mrts_obs_onehot_packed_dev(h.h, rows, self._p(packed), n_packed, cap, self._p(index), self._p(out),
                                                  self._s(stream)))
        return out

    def obs_pack_status(self):
        """(lossy_rows, bad_reads) since the last call of this (mrts_obs_packed_status): the rows pack_obs flagged
        lossy (cut at cap, a clamped value, a plane 5.. value other than 0 / 1) and the bad reads of unpack_obs /
        onehot_packed (an index outside the packed rows, a stored cell outside the map); clears both.  Synchronises."""
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.check(self._h.L.mrts_obs_packed_status(self._h.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def set_state_json(self, slot, text):
        """GameState.fromJSON into the game behind `slot`; call get_masks() before a policy reads masks."""
        super().set_state_json(slot, text)
        self._policy_stamp(None)

    def checkpoint(self):
        return self._host().checkpoint()

    def restore(self, data):
        """Every game's state from checkpoint(); call get_masks() before a policy reads masks."""
        self._host().restore(data)
        self._policy_stamp(None)

    @property
    def dims(self):
        h = self._h
        return h.S, h.H, h.W, h.C, h.K
