"""ForwardModel: the batched forward model for search AIs over the libmrts C ABI (mrts_copy_games / mrts_playout /
mrts_evaluate and their device forms).  GPU only, like DeviceVecEnv."""
import numpy as np

from . import _lib
from ._device import DeviceHandle
from .vec_client import UnitTypeTable, _Handle, _resolve


class ForwardModel(DeviceHandle):
    """Batched forward model for search AIs: n games kept in HBM, each advanced by
    NaiveMCTS.simulate (ai/mcts/naivemcts/NaiveMCTS.java:297-308) with its own playout policies
    (RandomBiasedAI / PassiveAI for players 0 and 1), cloned from any handle's games with
    GameState.clone() semantics (rts/GameState.java:591-610), and scored with
    SimpleSqrtEvaluationFunction3.  Game j's java.util.Random streams are seeded from seed + j (see
    DESIGN.md).  Device calls are ordered on torch's current stream of the device."""

    def __init__(self, n_games, map_path, policies=("RandomBiasedAI", "RandomBiasedAI"), utt=None, device=0, seed=0,
                 max_units=0):
        torch = self._open("ForwardModel", device)
        utt = utt or UnitTypeTable()
        p0, p1 = policies
        p0 = p0 if isinstance(p0, (list, tuple)) else [p0] * n_games
        p1 = p1 if isinstance(p1, (list, tuple)) else [p1] * n_games
        maps = list(map_path) if isinstance(map_path, (list, tuple)) else [map_path] * n_games  # one per game, same size
        self._h = _Handle(0, n_games, 1 << 30, [_resolve("", m) for m in maps], p1, utt, False, device, seed, 0,
                          ai1s=p0, forward_model=True, max_units=max_units)
        self.n = n_games
        self.value = torch.zeros(n_games, dtype=torch.float32, device=self.device)
        torch.cuda.synchronize(self.device)

    def reset(self):
        """Every game back to its map's initial state (random streams continue)."""
        h = self._h
        _lib.check(h.L.mrts_reset_dev(h.h, None, None, None, None, None, 0, self._s()))

    def copy_from(self, pairs, src=None):
        """gs[dst] = src_games[src_game].clone() for (dst, src_game) rows of `pairs` (int32 [n, 2]: a
        torch tensor on this device, or anything numpy accepts).  src: a DeviceVecEnv,
        JNIGridnetVecClient or ForwardModel with the same map size (None = self)."""
        h = self._h
        sh = h.h if src is None else src._h.h
        if isinstance(pairs, self.torch.Tensor) and pairs.is_cuda:
            assert pairs.dtype == self.torch.int32 and pairs.is_contiguous() and pairs.dim() == 2 and pairs.shape[1] == 2
            if src is not None and hasattr(src, "synchronize"):
                src.synchronize()
            _lib.check(h.L.mrts_copy_games_dev(h.h, sh, self._p(pairs), pairs.shape[0], self._s()))
        else:
            pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
            self.synchronize()
            _lib.check(h.L.mrts_copy_games(h.h, sh, pr.ctypes.data, pr.shape[0]))

    def playout(self, horizon):
        """NaiveMCTS.simulate(gs, gs.getTime() + horizon) on every game (one launch)."""
        if not -_lib.MRTS_MAX_HORIZON <= horizon <= _lib.MRTS_MAX_HORIZON:
            raise ValueError("horizon out of range")
        h = self._h
        _lib.check(h.L.mrts_playout_dev(h.h, int(horizon), self._s()))

    def trace_step(self, pairs, until, generic=False):
        """One entry of TestTracesIntegrity.testTrace (test/microrts/TestTracesIntegrity.java:72-127) on
        every game: issueSafe(player 0's rows), issueSafe(player 1's rows), then cycle() until time ==
        until[g].  pairs: int32 [n_games, n_pairs, 8] rows [player (-1 = padding), x, y, type, parameter,
        target x, target y, unit type].  Returns the MRTS_TRACE_* bits per game (int32 [n_games])."""
        h = self._h
        pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32))
        assert pr.ndim == 3 and pr.shape[0] == self.n and pr.shape[2] == 8
        un = np.ascontiguousarray(np.asarray(until, dtype=np.int32).reshape(self.n))
        out = np.zeros(self.n, dtype=np.int32)
        self.synchronize()
        _lib.check(h.L.mrts_trace_step(h.h, pr.ctypes.data, pr.shape[1], un.ctypes.data, out.ctypes.data, int(bool(generic))))
        return out

    def evaluate(self, maxplayer=0, out=None):
        """SimpleSqrtEvaluationFunction3.evaluate(maxplayer, 1 - maxplayer, gs): float32 [n] on device."""
        h = self._h
        out = self.value if out is None else out
        _lib.check(h.L.mrts_evaluate_dev(h.h, int(maxplayer), self._p(out), self._s()))
        return out

    # the state accessors of the shared base, under the parameter name this class has always given them
    def dump_state(self, game):
        return self._host().dump(game)

    def state_json(self, game):
        return self._host().state_json(game)

    def set_state_json(self, game, text):
        self._host().set_state_json(game, text)
