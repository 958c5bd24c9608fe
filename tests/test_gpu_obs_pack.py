"""Packed observation rows on the GPU (mrts_obs_pack_dev / _unpack_dev / _onehot_packed_dev / _packed_status;
DeviceVecEnv.pack_obs / unpack_obs / onehot_packed / obs_pack_status) against the numpy packer of
tests/obs_pack_ref.py and against the dense tensors a rollout saw.

One handle per shape, 8 slots, seed 3, random-policy steps; every step's env.obs is packed at cap = H*W and cloned
beside its onehot_obs:
  4x4 (16 cells: less than a wave, a one-word bitmap), 8x8 (one chunk), NoWhereToRun9x8 (72 cells: a short last
  chunk, odd row words, H*W*F no multiple of 16, 3-word bitmaps), 16x16 (four chunks, one tile), 32x32 partially
  observable (four tiles, 32-word bitmaps), 128x96 (cells above 2^13, 48 tiles; 5 steps)."""
import ctypes

import numpy as np
import pytest

from tests import obs_pack_ref as OR
from tests.gpu_support import ptr, torch_gpu

pytestmark = pytest.mark.gpu

S, SEED = 8, 0x0BADC0FFEE
CASES = {
    "4x4": ("maps/4x4/base4x4.xml", False, 40),
    "8x8": ("maps/8x8/basesWorkers8x8.xml", False, 40),
    "8x8-po": ("maps/8x8/basesWorkers8x8.xml", True, 40),
    "9x8": ("maps/NoWhereToRun9x8.xml", False, 40),
    "9x8-po": ("maps/NoWhereToRun9x8.xml", True, 40),
    "16x16": ("maps/16x16/basesWorkers16x16.xml", False, 40),
    "32x32-po": ("maps/BWDistantResources32x32.xml", True, 40),
    "128x96": ("maps/BroodWar/(2)HeartbreakRidge.scxA.xml", False, 5),
}


def _np32(t):
    return t.cpu().view(torch_gpu().int32).numpy().view(np.uint32)


def _u32(a, device):
    """a numpy uint32 array as a uint32 tensor on the device"""
    torch = torch_gpu()
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(device).view(torch.uint32)


def _filled(shape, device, word=0xDEADBEEF):
    torch = torch_gpu()
    return torch.full(shape, word - (1 << 32) if word >> 31 else word, dtype=torch.int32, device=device).view(torch.uint32)


def _rollout(env, steps, each):
    env.reset()
    each(0)
    for k in range(steps):
        env.random_policy(SEED, k)
        env.step()
        each(k + 1)


class Case:
    """one shape: a rollout whose every step is kept packed (cap = H*W), as int32 planes and one-hot"""

    def __init__(self, name):
        torch = torch_gpu()
        from microrts_amd import DeviceVecEnv

        path, po, steps = CASES[name]
        big, self.po = name == "128x96", po
        self.env = env = DeviceVecEnv(S, 0, 2000, [path] * S, seed=3, partial_obs=po, max_units=1024 if big else 0)
        _, self.H, self.W, self.C, _ = env.dims
        self.HW, self.T = self.H * self.W, steps + 1
        self.buf = env.obs_packed_buffer(self.T, cap=self.HW)
        obs, hot = [], []

        def each(t):
            env.pack_obs(self.buf[t])
            obs.append(env.obs.clone())
            hot.append(env.onehot_obs())
        _rollout(env, steps, each)
        self.obs, self.hot = torch.stack(obs), torch.stack(hot)  # [T][S]...
        self.F = self.hot.shape[-1]
        assert not env.error_flags().any()
        self.status = env.obs_pack_status()

    def dense_onehot(self, obs):
        """onehot_obs (the dense kernel) of any number of rows, S at a time"""
        torch = torch_gpu()
        n = obs.shape[0]
        pad = torch.cat([obs, obs.new_zeros(((-n) % S,) + tuple(obs.shape[1:]))]).contiguous()
        return torch.cat([self.env.onehot_obs(obs=pad[i:i + S]) for i in range(0, pad.shape[0], S)])[:n]


_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


@pytest.fixture(params=list(CASES))
def case(request):
    return _case(request.param)


def test_packed_words_equal_the_numpy_packer(case):
    env = case.env
    assert case.C == (8 if case.po else 6)
    assert env.obs_packed_words(case.HW) == OR.words(case.C, case.HW, case.HW) == case.buf.shape[-1]
    want = OR.pack(case.obs.cpu().numpy().reshape(case.T * S, case.C, case.HW), case.HW)
    got = _np32(case.buf).reshape(case.T * S, -1)
    assert (want[:, 0] > 0).all() and not (want[:, 0] & OR.LOSSY).any()
    assert np.array_equal(got, want)
    assert (case.obs[1:] != case.obs[:-1]).any(), "a rollout in which nothing moved"
    assert case.status == (0, 0)


def test_readers_give_back_what_the_network_saw(case):
    torch = torch_gpu()
    env = case.env
    assert torch.equal(env.unpack_obs(case.buf).reshape(case.obs.shape), case.obs)
    assert torch.equal(env.onehot_packed(case.buf).reshape(case.hot.shape), case.hot)
    # a gather index with repeats over all T * S rows, into buffers that held something else
    N = case.T * S
    g = torch.Generator().manual_seed(case.HW)
    idx = torch.cat([torch.randint(0, N, (19,), generator=g), torch.tensor([N - 1, 0, 5, 5])]).to(torch.int32)
    li = idx.long().to(env.device)
    o = torch.full((idx.numel(), case.C, case.H, case.W), -7, dtype=torch.int32, device=env.device)
    assert env.unpack_obs(case.buf, index=idx.to(env.device), out=o) is o
    assert torch.equal(o, case.obs.reshape(N, case.C, case.H, case.W)[li])
    h = torch.full((idx.numel(), case.H, case.W, case.F), 9, dtype=torch.uint8, device=env.device)
    assert env.onehot_packed(case.buf, index=idx.to(env.device), out=h) is h
    assert torch.equal(h, case.hot.reshape(N, case.H, case.W, case.F)[li])
    assert env.obs_pack_status() == (0, 0)


def test_default_cap_holds_a_16x16_rollout():
    torch = torch_gpu()
    from microrts_amd import DeviceVecEnv

    env = DeviceVecEnv(S, 0, 2000, [CASES["16x16"][0]] * S, seed=3)
    T = 61
    buf = env.obs_packed_buffer(T)
    assert buf.shape == (T, S, 265) and env.obs_packed_words() == 265 and env.obs_packed_words(64) == 137
    obs = []

    def each(t):
        env.pack_obs(buf[t])
        obs.append(env.obs.clone())
    _rollout(env, T - 1, each)
    assert env.obs_pack_status() == (0, 0)
    assert torch.equal(env.unpack_obs(buf).reshape(T, S, 6, 16, 16), torch.stack(obs))
    assert np.array_equal(_np32(buf).reshape(T * S, -1), OR.pack(torch.stack(obs).cpu().numpy().reshape(T * S, 6, 256), 128))
    env.close()


def test_synthetic_rows_through_all_three_kernels(case):
    torch = torch_gpu()
    env, H, W, C, HW = case.env, case.H, case.W, case.C, case.HW
    syn, names, info = OR.synthetic_rows(H, W, C, seed=HW)
    n = len(names)
    d_syn = torch.from_numpy(syn).to(env.device)
    hot_of_tensor = case.dense_onehot(d_syn)
    assert np.array_equal(hot_of_tensor.cpu().numpy(), OR.onehot(syn, 7)), "onehot_obs against the numpy encoding"
    assert env.obs_pack_status() == (0, 0)
    for cap in (HW, OR.synthetic_cap(H, W), 1):
        want = OR.pack(syn, cap)
        out = _filled((n, env.obs_packed_words(cap)), env.device)
        env.pack_obs(out, obs=d_syn)
        assert np.array_equal(_np32(out), want), f"cap {cap}"
        flagged = (want[:, 0] & OR.LOSSY) != 0
        assert np.array_equal(flagged, OR.flagged(info, names, cap))
        assert env.obs_pack_status() == (int(flagged.sum()), 0), f"cap {cap}"
        kept = OR.unpack(want, C, H, W, cap)
        got = env.unpack_obs(out).cpu().numpy()
        assert np.array_equal(got, kept), f"cap {cap}"
        assert np.array_equal(got[~flagged], syn[~flagged])
        hot = env.onehot_packed(out)
        assert np.array_equal(hot.cpu().numpy(), OR.onehot(kept, 7)), f"cap {cap}"
        # every row that was not cut, clamped values included: the one-hot of the tensor that was packed
        whole = torch.from_numpy((want[:, 0] & (OR.LOSSY - 1)) <= cap).to(env.device)
        assert int(whole.sum()) >= (n - 3 if cap > 1 else 15) and torch.equal(hot[whole], hot_of_tensor[whole]), f"cap {cap}"
        clamped_only = [i for i, k in enumerate(names) if info[k][1] and info[k][0] <= cap]
        assert len(clamped_only) == 7 and flagged[clamped_only].all() and bool(whole[clamped_only].all())
    # a view at an odd word offset of a larger buffer: only its own words are written
    cap = 3
    big = _filled((3, n, env.obs_packed_words(cap)), env.device, word=7)
    env.pack_obs(big[1], obs=d_syn, cap=cap)
    assert np.array_equal(_np32(big[1]), OR.pack(syn, cap)) and (_np32(big[0]) == 7).all() and (_np32(big[2]) == 7).all()
    env.obs_pack_status()


def test_reader_bounds(case):
    """The readers' bounds handling (k_obs_unpack / k_obs_onehot_packed: obsPackedRow refuses an index outside the
    packed rows before any read of it, obsScatter skips a stored cell >= H*W before any LDS write, the stored count is
    clamped to cap): zero rows, the row without the bad cell, and the two counted."""
    torch = torch_gpu()
    env, H, W, C, HW = case.env, case.H, case.W, case.C, case.HW
    assert HW < 1 << 16  # the cell number H*W fits the 16-bit field
    syn, names, _ = OR.synthetic_rows(H, W, C, seed=HW)
    k = names.index("exactly_cap")
    cap = HW
    rows = OR.pack(syn[[k, names.index("cell_last")]], cap)
    n0 = int(rows[0, 0])
    bad = rows.copy()
    bad[0, 0] = n0 + 1
    bad[0, 1 + 2 * n0] = HW | 2 << 16 | 5 << 18 | 6 << 21  # a cell just outside the map, with every field set
    bad[0, 2 + 2 * n0] = 3 | 9 << 16
    d_bad = _u32(bad, env.device)
    N = bad.shape[0]
    idx = torch.tensor([0, -1, 1, N, 0], dtype=torch.int32, device=env.device)
    want = OR.unpack(rows, C, H, W, cap)[[0, 0, 1, 1, 0]]
    want[[1, 3]] = 0
    assert env.obs_pack_status() == (0, 0)
    o = torch.full((5, C, H, W), -7, dtype=torch.int32, device=env.device)
    env.unpack_obs(d_bad, index=idx, out=o)
    assert np.array_equal(o.cpu().numpy(), want)
    assert env.obs_pack_status() == (0, 4)  # two indices, the bad cell read twice
    hot = torch.full((5, H, W, case.F), 9, dtype=torch.uint8, device=env.device)
    env.onehot_packed(d_bad, index=idx, out=hot)
    hw = OR.onehot(want, 7)
    hw[[1, 3]] = 0
    assert np.array_equal(hot.cpu().numpy(), hw)
    assert env.obs_pack_status() == (0, 4)
    # a stored count above cap (junk included) reads cap cells: the words of the row, nothing past them
    cut = OR.pack(syn, OR.synthetic_cap(H, W))
    cut[:, 0] |= 0x7FFF0000
    c2 = OR.synthetic_cap(H, W)
    got = env.unpack_obs(_u32(cut, env.device)).cpu().numpy()
    full = np.array([min(n, c2) == c2 for n in (OR.pack(syn, c2)[:, 0] & (OR.LOSSY - 1))])
    assert np.array_equal(got[full], OR.unpack(cut, C, H, W, c2)[full])
    env.obs_pack_status()


def test_refusals():
    """every ValueError of the Python layer and every -EINVAL of the C calls"""
    torch = torch_gpu()
    from microrts_amd import _lib

    case = _case("8x8")
    env, dev = case.env, case.env.device
    L, h = _lib.load(), env._h.h
    W8 = env.obs_packed_words(8)
    assert W8 == 1 + 16 + 2 and L.mrts_obs_packed_words(h, 8) == W8 and L.mrts_obs_packed_words(h, 64) == 131
    pk = torch.zeros((S, W8), dtype=torch.int32, device=dev).view(torch.uint32)
    ob = torch.zeros((S, 6, 8, 8), dtype=torch.int32, device=dev)
    hot = torch.zeros((S * 64 * 29 + 16,), dtype=torch.uint8, device=dev)
    a, b = ctypes.c_int64(0), ctypes.c_int64(0)

    def calls(hh, n=S, cap=8, packed=pk, obs=ob, out=hot, n_packed=S):
        return [L.mrts_obs_pack_dev(hh, n, ptr(obs), cap, ptr(packed), None),
                L.mrts_obs_unpack_dev(hh, n, ptr(packed), n_packed, cap, None, ptr(obs), None),
                L.mrts_obs_onehot_packed_dev(hh, n, ptr(packed), n_packed, cap, None, ptr(out), None)]

    assert calls(h) == [0, 0, 0]
    assert calls(None) == [-22] * 3 and L.mrts_last_error().decode() == "null handle"
    assert L.mrts_obs_packed_words(None, 8) == -22 and L.mrts_obs_packed_status(None, ctypes.byref(a), ctypes.byref(b)) == -22
    assert calls(h, n=-1) == [-22] * 3 and "n_rows" in L.mrts_last_error().decode()
    for cap in (0, 65, -1):
        assert L.mrts_obs_packed_words(h, cap) == -22
        assert calls(h, cap=cap) == [-22] * 3 and "cap" in L.mrts_last_error().decode()
    assert calls(h, packed=None) == [-22] * 3 and calls(h, obs=None)[:2] == [-22] * 2 and calls(h, out=None)[2] == -22
    assert calls(h, n_packed=0)[1:] == [-22] * 2 and calls(h, n_packed=S - 1)[1:] == [-22] * 2
    assert L.mrts_obs_onehot_packed_dev(h, S, ptr(pk), S, 8, None, ctypes.c_void_p(hot.data_ptr() + 1), None) == -22
    assert "misaligned" in L.mrts_last_error().decode()
    assert L.mrts_obs_pack_dev(h, S, ptr(ob), 8, ctypes.c_void_p(pk.data_ptr() + 2), None) == -22
    assert L.mrts_obs_unpack_dev(h, S, ptr(pk), S, 8, None, ctypes.c_void_p(ob.data_ptr() + 2), None) == -22
    assert L.mrts_obs_packed_status(h, None, ctypes.byref(b)) == -22 and L.mrts_obs_packed_status(h, ctypes.byref(a), None) == -22
    assert L.mrts_obs_packed_status(h, ctypes.byref(a), ctypes.byref(b)) == 0 and (a.value, b.value) == (0, 0)
    # the Python layer names the argument
    for bad in (0, 65, True, 2.0):
        with pytest.raises(ValueError, match="cap"):
            env.obs_packed_buffer(2, cap=bad)
    with pytest.raises(ValueError, match="out"):
        env.pack_obs(pk.view(torch.int32))  # dtype
    with pytest.raises(ValueError, match="out"):
        env.pack_obs(torch.zeros((S, W8 + 1), dtype=torch.int32, device=dev).view(torch.uint32))  # no cap has these words
    with pytest.raises(ValueError, match="out"):
        env.pack_obs(pk, cap=9)
    with pytest.raises(ValueError, match="out"):
        env.pack_obs(env.obs_packed_buffer(2, cap=8))  # [T][S][words]: one step at a time
    with pytest.raises(ValueError, match="out"):
        env.pack_obs(pk.cpu())
    with pytest.raises(ValueError, match="obs"):
        env.pack_obs(pk, obs=ob[:4])
    with pytest.raises(ValueError, match="obs"):
        env.pack_obs(pk, obs=ob.to(torch.int64))
    with pytest.raises(ValueError, match="obs"):
        env.pack_obs(pk, obs=ob.permute(0, 1, 3, 2))
    for read in (env.unpack_obs, env.onehot_packed):
        with pytest.raises(ValueError, match="packed"):
            read(pk.view(torch.int32))
        with pytest.raises(ValueError, match="packed"):
            read(torch.zeros((S, 2 * W8), dtype=torch.int32, device=dev).view(torch.uint32)[:, ::2])
        with pytest.raises(ValueError, match="packed"):
            read(pk[:0])
        with pytest.raises(ValueError, match="index"):
            read(pk, index=torch.zeros(3, dtype=torch.int64, device=dev))
        with pytest.raises(ValueError, match="index"):
            read(pk, index=torch.zeros((3, 1), dtype=torch.int32, device=dev))
        with pytest.raises(ValueError, match="index"):
            read(pk, index=torch.zeros(3, dtype=torch.int32))
        with pytest.raises(ValueError, match="out"):
            read(pk, out=torch.zeros((S, 6, 8, 8), dtype=torch.float32, device=dev))
    assert env.obs_pack_status() == (0, 0)
