"""Host-side mirror of the reference's env-client interface over the libmrts C ABI.

* ``JNIGridnetVecClient`` mirrors ``tests.JNIGridnetVecClient`` (reference
  src/tests/JNIGridnetVecClient.java:17-335): same constructor arguments, ``reset`` / ``gameStep``
  / ``getMasks`` / ``close``, host numpy arrays that are library-owned views reused by the next
  call (like the Java ``Response`` buffers, GameState.java:923-925).
* ``_Handle`` owns one mrts_env and its host-side accessors; ``DeviceVecEnv`` (device_env.py, the
  zero-copy rollout form) and ``ForwardModel`` (forward_model.py) are built on it too.

There is no CPU fallback: constructing the client without a GPU or without libmrts.so raises.
"""
import ctypes
import os

import numpy as np

from . import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class UnitTypeTable:
    """rts.units.UnitTypeTable(version, crs) (src/rts/units/UnitTypeTable.java:22-349)."""

    EMPTY_TYPE_TABLE = -1
    VERSION_ORIGINAL = 1
    VERSION_ORIGINAL_FINETUNED = 2
    VERSION_NON_DETERMINISTIC = 3
    MOVE_CONFLICT_RESOLUTION_CANCEL_BOTH = 1
    MOVE_CONFLICT_RESOLUTION_CANCEL_RANDOM = 2
    MOVE_CONFLICT_RESOLUTION_CANCEL_ALTERNATING = 3

    def __init__(self, version=VERSION_ORIGINAL, crs=MOVE_CONFLICT_RESOLUTION_CANCEL_BOTH):
        if version not in (1, 2, 3) or crs not in (1, 2, 3):
            raise ValueError("unsupported UnitTypeTable version / conflict policy")
        self.version, self.crs = version, crs
        self.json = None  # set by fromJSON: the table is then the JSON's (version / crs unused)
        self._desc = None

    @classmethod
    def fromJSON(cls, text):
        """UnitTypeTable.fromJSON (UnitTypeTable.java:414-433), validated by the native parser (its
        quirks included: harvestTime is read from "produceTime", returnTime is not read)."""
        utt = cls()
        utt.json = text if isinstance(text, str) else text.decode()
        utt.toJSON()  # raises on a table this build cannot run
        return utt

    def toJSON(self):
        """UnitTypeTable.toJSON (UnitTypeTable.java:372-383), byte for byte."""
        L = _lib.load()
        j = self.json.encode() if self.json else None
        n = L.mrts_utt_json(self.version, self.crs, j, None, 0)
        if n >= 0 or n == -22 or n == -95:
            raise ValueError(L.mrts_last_error().decode() or "invalid unit-type table")
        buf = ctypes.create_string_buffer(-n)
        _lib.check(0 if L.mrts_utt_json(self.version, self.crs, j, buf, -n) >= 0 else -1)
        return buf.value.decode()

    def _table(self):
        if self._desc is None:
            import json

            self._desc = json.loads(self.toJSON())
        return self._desc

    @property
    def TYPES(self):
        return [t["name"] for t in self._table()["unitTypes"]]

    def getUnitTypes(self):
        return self._table()["unitTypes"]

    def getMoveConflictResolutionStrategy(self):
        return self._table()["moveConflictResolutionStrategy"]

    def getMaxAttackRange(self):
        """UnitTypeTable.getMaxAttackRange (:341-349)."""
        return max(t["attackRange"] for t in self._table()["unitTypes"])


class _ClientView:
    """The per-env client objects the Java VecClient exposes (clients / selfPlayClients); only
    sendUTT() (JNIGridnetClient.java:225-233) is meaningful on this build."""

    def __init__(self, utt):
        self._utt = utt

    def sendUTT(self):
        return self._utt.toJSON()


class Responses:
    """ai.jni.Responses (src/ai/jni/Responses.java:12-30)."""

    def __init__(self, observation, reward, done):
        self.observation, self.reward, self.done = observation, reward, done


def _bot_kind(ai):
    name = ai if isinstance(ai, str) else (ai.__name__ if isinstance(ai, type) else type(ai).__name__)
    if name in ("PassiveAI", "passive"):
        return _lib.MRTS_BOT_PASSIVE
    if name in ("RandomBiasedAI", "random_biased"):
        return _lib.MRTS_BOT_RANDOM_BIASED
    if name in ("LightRush", "lightRushAI", "light_rush"):  # ai.abstraction.LightRush(utt): A* pathfinding
        return _lib.MRTS_BOT_LIGHT_RUSH
    raise NotImplementedError(f"opponent AI {name!r} has no native implementation "
                              "(only PassiveAI / RandomBiasedAI / LightRush)")


def _check_rfs(rfs):
    """a_rfs (RewardFunctionInterface[], :106) -> MRTS_RF_* ids: class names or instances/classes with
    those names (src/ai/reward/*.java); None = [WinLossRewardFunction]."""
    out = []
    for r in (rfs or ["WinLossRewardFunction"]):
        name = r if isinstance(r, str) else (r.__name__ if isinstance(r, type) else type(r).__name__)
        name = name.rsplit(".", 1)[-1]
        if name not in _lib.REWARD_FUNCTIONS:
            raise NotImplementedError(f"reward function {name!r} is not implemented on the GPU path "
                                      f"(available: {sorted(_lib.REWARD_FUNCTIONS)})")
        out.append(_lib.REWARD_FUNCTIONS[name])
    if len(out) > 8:
        raise ValueError("at most 8 reward functions")
    return out


def _kinds(ais, n):
    kinds = [_bot_kind(a) for a in (ais or [])][:n]
    kinds += [_lib.MRTS_BOT_PASSIVE] * (n - len(kinds))
    return (ctypes.c_int32 * max(1, n))(*(kinds or [0]))


def _last_map_index(n_selfplay, n_bot):
    """The largest a_mapPaths index Java reads: mapPaths[i*2] per self-play client
    (JNIGridnetVecClient.java:119), mapPaths[a_num_selfplayenvs + i] per bot env (:123), and
    mapPaths[0] for the storage sizing (:127)."""
    return max([0] + ([2 * (n_selfplay // 2 - 1)] if n_selfplay >= 2 else []) +
               ([n_selfplay + n_bot - 1] if n_bot > 0 else []))


class _Handle:
    def __init__(self, n_selfplay, n_bot, max_steps, map_paths, ai2s, utt, partial_obs, device, seed, slot_id_base,
                 ai1s=None, mask_delta=False, rewards=None, forward_model=False, max_units=0):
        need = _last_map_index(n_selfplay, n_bot)
        if len(map_paths) <= need:
            raise ValueError(f"{len(map_paths)} map paths; Java reads mapPaths[{need}]")
        L = _lib.load()
        self.L = L
        self._paths = (ctypes.c_char_p * len(map_paths))(*[p.encode() for p in map_paths])
        self._kinds = _kinds(ai2s, n_bot)
        self._ai1 = _kinds(ai1s, n_bot) if ai1s is not None else None
        P32 = ctypes.POINTER(ctypes.c_int32)
        self.rewards = list(rewards) if rewards else [0]
        self._rk = (ctypes.c_int32 * len(self.rewards))(*self.rewards)
        self.R = len(self.rewards)
        cfg = _lib.MrtsConfig(n_selfplay, n_bot, max_steps, int(bool(partial_obs)), utt.version, utt.crs,
                              ctypes.cast(self._kinds, P32),
                              ctypes.cast(self._ai1, P32) if self._ai1 is not None else None,
                              ctypes.cast(self._paths, ctypes.POINTER(ctypes.c_char_p)), device, seed, slot_id_base,
                              int(bool(mask_delta)), ctypes.cast(self._rk, P32), self.R, int(bool(forward_model)),
                              utt.json.encode() if utt.json else None, int(max_units))
        h = ctypes.c_void_p()
        _lib.check(L.mrts_create(ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        d = [ctypes.c_int32() for _ in range(5)]
        L.mrts_dims(self.h, *[ctypes.byref(x) for x in d])
        self.S, self.H, self.W, self.C, self.K = [x.value for x in d]

    def close(self):
        if getattr(self, "h", None):
            self.L.mrts_destroy(self.h)
            self.h = None

    def dump(self, slot):
        buf = np.zeros(1 << 16, np.int32)
        n = self.L.mrts_get_state(self.h, slot, buf.ctypes.data_as(ctypes.c_void_p), buf.size)
        if n < 0:
            raise RuntimeError(self.L.mrts_last_error().decode())
        return buf[:n].copy()

    def error_flags(self):
        f = np.zeros(self.S, np.uint32)
        _lib.check(self.L.mrts_error_flags(self.h, f.ctypes.data_as(ctypes.c_void_p)))
        return f

    def state_json(self, slot):
        n = self.L.mrts_get_state_json(self.h, slot, None, 0)  # -(length + 1), or an errno
        if n > -64:
            _lib.check(n if n < 0 else -22)
        buf = ctypes.create_string_buffer(-n)
        n = self.L.mrts_get_state_json(self.h, slot, buf, -n)
        _lib.check(0 if n >= 0 else n)
        return buf.value.decode()

    def set_state_json(self, slot, text):
        _lib.check(self.L.mrts_set_state_json(self.h, slot, text.encode() if isinstance(text, str) else text))

    def checkpoint(self):
        n = self.L.mrts_checkpoint_size(self.h)
        buf = ctypes.create_string_buffer(n)
        _lib.check(self.L.mrts_checkpoint(self.h, buf, n))
        return buf.raw

    def restore(self, data):
        _lib.check(self.L.mrts_restore(self.h, ctypes.c_char_p(bytes(data)), len(data)))

    def env_steps(self):
        f = np.zeros(self.S, np.int32)
        _lib.check(self.L.mrts_env_steps(self.h, f.ctypes.data_as(ctypes.c_void_p)))
        return f


def _resolve(micrortsPath, p):
    if micrortsPath:
        return os.path.join(micrortsPath, p)
    return p if os.path.isabs(p) or os.path.exists(p) else os.path.join(ROOT, p)


class JNIGridnetVecClient:
    """tests.JNIGridnetVecClient (src/tests/JNIGridnetVecClient.java:106-142) on MI355X."""

    def __init__(self, a_num_selfplayenvs, a_num_envs, a_max_steps, a_rfs, a_micrortsPath, a_mapPaths, a_ai2s=None,
                 a_utt=None, partial_obs=False, device=0, seed=0, slot_id_base=0, _ai1s=None):
        rewards = _check_rfs(a_rfs)
        # Java indexes a_ai2s[i] (and a_ai1s[i] in the bot-only constructor) for every bot env
        # (JNIGridnetVecClient.java:121-123,163-165) and throws on a null or short array; no silent
        # PassiveAI default here (DeviceVecEnv keeps one, documented there)
        for name, ais in (("a_ai2s", a_ai2s), ("a_ai1s", _ai1s)):
            if (name == "a_ai2s" or _ai1s is not None) and a_num_envs > 0 and (ais is None or len(ais) < a_num_envs):
                raise ValueError(f"{name} names {0 if ais is None else len(ais)} bots for {a_num_envs} bot environments")
        utt = a_utt or UnitTypeTable()
        paths = [_resolve(a_micrortsPath, p) for p in a_mapPaths]
        self._h = _Handle(a_num_selfplayenvs, a_num_envs, a_max_steps, paths, a_ai2s, utt, partial_obs, device, seed,
                          slot_id_base, ai1s=_ai1s, rewards=rewards)
        self.botOnly = _ai1s is not None
        self.maxSteps = a_max_steps
        self.utt = utt
        self.partialObs = partial_obs
        self.mapPaths = list(a_mapPaths)
        h = self._h
        self.num_slots, self.height, self.width, self.num_planes, self.mask_slots = h.S, h.H, h.W, h.C, h.K
        self._resp = _lib.MrtsResponses()
        # the Java fields of per-env clients (:22-26); each offers sendUTT()
        self.selfPlayClients = [_ClientView(utt)] * (a_num_selfplayenvs // 2)
        self.clients = [_ClientView(utt)] * a_num_envs

    def sendUTT(self):
        """The unit-type table as JSON (JNIGridnetClient.sendUTT, :225-233)."""
        return self.utt.toJSON()

    def getGameStateJSON(self, slot):
        """GameState.toJSON of the game behind `slot` (unit IDs = list positions)."""
        return self._h.state_json(slot)

    def setGameStateJSON(self, slot, text):
        """GameState.fromJSON into the game behind `slot` (envSteps restarts at 0)."""
        self._h.set_state_json(slot, text)

    def checkpoint(self):
        """bytes holding every game's state (random streams and envSteps included)."""
        return self._h.checkpoint()

    def restore(self, data):
        self._h.restore(data)

    @classmethod
    def bots(cls, a_max_steps, a_rfs, a_micrortsPath, a_mapPaths, a_ai1s, a_ai2s, a_utt=None, partial_obs=False, device=0,
             seed=0, slot_id_base=0):
        """The bot-only constructor JNIGridnetVecClient(maxSteps, rfs, path, mapPaths, ai1s, ai2s, utt, po)
        (src/tests/JNIGridnetVecClient.java:157-177): JNIBotClients, reward/done only."""
        return cls(0, len(a_ai2s), a_max_steps, a_rfs, a_micrortsPath, a_mapPaths, a_ai2s, a_utt, partial_obs, device, seed,
                   slot_id_base, _ai1s=list(a_ai1s))

    def _responses(self):
        h, r = self._h, self._resp
        obs = None if getattr(self, "botOnly", False) else np.ctypeslib.as_array(r.obs, shape=(h.S, h.C, h.H, h.W))
        rew = np.ctypeslib.as_array(r.reward, shape=(h.S, h.R))
        done = np.ctypeslib.as_array(r.done, shape=(h.S, h.R)).view(np.bool_)
        return Responses(obs, rew, done)

    def reset(self, players=None):
        """reset(int[] players) (:179-211)."""
        p = None if players is None else np.ascontiguousarray(players, np.int32)
        _lib.check(self._h.L.mrts_reset(self._h.h, None if p is None else p.ctypes.data_as(ctypes.c_void_p),
                                        ctypes.byref(self._resp)))
        return self._responses()

    def gameStep(self, action, players=None):
        """gameStep(int[][][] action, int[] players) (:213-297).

        action is either the Java layout [slots][n_rows][8] (rows [pos, 7 components], any order,
        duplicates allowed: PlayerAction.fromVectorAction list semantics) or the grid layout
        [slots][H*W][7] (row r = cell r, ascending — what MicroRTS-Py sends)."""
        h = self._h
        if action is None:  # bot-only clients take no actions (JNIGridnetVecClient.java:214-216)
            action = np.zeros((h.S, h.H * h.W, 7), np.int32)
        a = np.ascontiguousarray(action, np.int32)
        p = None if players is None else np.ascontiguousarray(players, np.int32)
        pp = None if p is None else p.ctypes.data_as(ctypes.c_void_p)
        if a.ndim == 3 and a.shape[0] == h.S and a.shape[2] == 8:
            _lib.check(h.L.mrts_step_rows(h.h, a.ctypes.data_as(ctypes.c_void_p), a.shape[1], pp, ctypes.byref(self._resp)))
        else:
            a = a.reshape(h.S, h.H * h.W, 7)
            _lib.check(h.L.mrts_step(h.h, a.ctypes.data_as(ctypes.c_void_p), pp, ctypes.byref(self._resp)))
        return self._responses()

    def getMasks(self, player=0, dtype=np.uint8, copy=True):
        """getMasks(int player) (:307-316) → [slots][H][W][79]; dtype np.int32 gives the Java int[][][][]
        element type.  copy=False returns a view of a library-owned pinned array that the next call
        refills (the Java client reuses its mask array the same way, JNIGridnetClient.java:211-215) —
        the fast form: the device-to-host copy runs at pinned-memory rate."""
        h = self._h
        if not copy:
            i32 = np.dtype(dtype) == np.int32
            ptr = ctypes.c_void_p()
            fn = h.L.mrts_get_masks_i32_host if i32 else h.L.mrts_get_masks_host
            _lib.check(fn(h.h, player, ctypes.byref(ptr)))
            ct = ctypes.c_int32 if i32 else ctypes.c_uint8
            return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ct)), shape=(h.S, h.H, h.W, h.K))
        if np.dtype(dtype) == np.int32:
            m = np.empty((h.S, h.H, h.W, h.K), np.int32)
            _lib.check(h.L.mrts_get_masks_i32(h.h, player, m.ctypes.data_as(ctypes.c_void_p)))
            return m
        m = np.empty((h.S, h.H, h.W, h.K), np.uint8)
        _lib.check(h.L.mrts_get_masks(h.h, player, m.ctypes.data_as(ctypes.c_void_p)))
        return m

    @property
    def envSteps(self):
        return self._h.env_steps()

    def dump_state(self, slot):
        return self._h.dump(slot)

    def error_flags(self):
        return self._h.error_flags()

    def close(self):
        """close() (:318-334)."""
        self._h.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

