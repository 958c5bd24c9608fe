"""Calls the Python package refuses before it touches the library: bad tensors, caps and indices handed to the policy
head, the packed policy rows and the packed observation rows, as (name, match, call) triples per group.  `match` is
what the tests' pytest.raises(..., match=) asks of the text; tests/test_python_refusals_cpu.py compares each case's
exception type and full text with tests/golden/python_refusals_parent.json, which this module recorded from the
package of the commit before the binding got its one packed-row check:

    python -m tests.python_refusal_cases tests/golden/python_refusals_parent.json

(run in a checkout of that commit, with this file copied in).  No case needs a GPU or a handle: the envs are
stand-ins that carry dims and a device, and the DeviceVecEnv methods are called unbound on stand-ins whose `_h` holds
sizes only, so a method that reached for the library instead of refusing would fail on the missing attribute.  Test
infrastructure only."""
import json
import sys
import types

W8 = 1 + 8 * 5  # words of a packed policy row of cap 8


def cases():
    """group -> [(name, match, call)]; every call raises"""
    import torch

    from microrts_amd import DeviceVecEnv, obs_pack, policy_head

    cpu = torch.device("cpu")
    dims = (4, 4, 4, 27, 79)
    env = types.SimpleNamespace(dims=dims, device=cpu)
    cuda = types.SimpleNamespace(dims=dims, device=torch.device("cuda", 0))
    lg = torch.zeros((4, 16, 78))
    mk = torch.zeros((4, 4, 4, 79), dtype=torch.uint8)
    ac = torch.zeros((4, 16, 7), dtype=torch.int32)
    out = torch.zeros((4, W8), dtype=torch.uint32)
    src = torch.zeros((4, 1), dtype=torch.int32)
    idx = torch.zeros(4, dtype=torch.int32)
    sizes = types.SimpleNamespace(S=4, H=4, W=4, C=27, K=79)
    g = {}

    # -- the dense head: check_head_args, evaluate_actions ---------------------------------------------------------
    head = [("logits", "float64", (lg.double(), mk, ac)), ("logits", "79 fields", (torch.zeros((4, 16, 79)), mk, ac)),
            ("logits", "transposed", (torch.zeros((4, 78, 16)).transpose(1, 2), mk, ac)),
            ("logits", "numpy", (lg.numpy(), mk, ac)), ("masks", "bool", (lg, mk.bool(), ac)),
            ("masks", "3 rows", (lg, mk[:3], ac)), ("actions", "int64", (lg, mk, ac.long())),
            ("actions", "a slice", (lg, mk, torch.zeros((4, 16, 8), dtype=torch.int32)[:, :, :7]))]
    g["head"] = [(f"check_head_args: {m} {what}", m, lambda a=a: policy_head.check_head_args(env, *a)) for m, what, a in head]
    g["head"] += [
        # the slot count is fixed for sample_actions
        ("check_head_args: 3 rows of logits for n=4", "logits", lambda: policy_head.check_head_args(env, lg[:3], mk, ac, n=4)),
        ("evaluate_actions: cpu tensors for a cuda env", "logits: on cpu", lambda: policy_head.evaluate_actions(cuda, lg, mk, ac)),
    ]

    # -- packed policy rows: packed_words, DeviceVecEnv.pack_step, check_pack_args, evaluate_actions_packed --------
    g["packed_words"] = [(f"policy_head.packed_words: cap {bad!r}", "cap", lambda bad=bad: policy_head.packed_words(env, bad))
                         for bad in (0, -1, 17, 2.0, True, "8")]

    def fake(**kw):  # what pack_step / pack_obs / the readers touch of a DeviceVecEnv before the library
        d = dict(dims=dims, device=cpu, masks=mk, actions=ac, source=src, obs=torch.zeros((4, 27, 4, 4), dtype=torch.int32),
                 torch=torch, _h=sizes)
        d.update(kw)
        return types.SimpleNamespace(**d)

    step = [("out", "int32", dict(out=out.to(torch.int32))), ("out", "one word more", dict(out=torch.zeros((4, W8 + 1), dtype=torch.uint32))),
            ("out", "cap 17 of 16 cells", dict(out=torch.zeros((4, 1 + 17 * 5), dtype=torch.uint32))),
            ("out", "cap 7 for cap 8's words", dict(out=out, cap=7)), ("cap", "cap 0", dict(out=out, cap=0)),
            ("out", "a slice", dict(out=torch.zeros((4, 2 * W8), dtype=torch.uint32)[:, :W8])),
            ("out", "3-D", dict(out=out.reshape(2, 2, W8))), ("out", "numpy", dict(out=out.numpy())),
            ("masks", "bool", dict(out=out, masks=mk.bool(), actions=ac)), ("masks", "3 rows", dict(out=out, masks=mk[:3], actions=ac)),
            ("actions", "int64", dict(out=out, actions=ac.long())),
            ("actions", "a slice", dict(out=out, actions=torch.zeros((4, 16, 8), dtype=torch.int32)[:, :, :7]))]
    g["pack_step"] = [(f"pack_step: {m} {what}", m, lambda kw=kw: DeviceVecEnv.pack_step(fake(), **kw)) for m, what, kw in step]
    g["pack_step"] += [
        ("pack_step: an env without masks", "masks", lambda: DeviceVecEnv.pack_step(fake(masks=None), out)),
        ("check_pack_args: source int64", "source", lambda: policy_head.check_pack_args(env, out, mk, ac, src.long())),
    ]

    big = types.SimpleNamespace(dims=(4, 256, 256, 27, 79), device=torch.device("meta"))
    n_big = (1 << 31) // (256 * 256)
    ev = [("logits", "float64", (lg.double(), out, None)), ("logits", "79 fields", (torch.zeros((4, 16, 79)), out, None)),
          ("logits", "numpy", (lg.numpy(), out, None)), ("logits", "transposed", (torch.zeros((4, 78, 16)).transpose(1, 2), out, None)),
          ("packed", "int32", (lg, out.to(torch.int32), None)), ("packed", "3 rows, no index", (lg, out[:3], None)),
          ("packed", "one word short", (lg, out[:, :W8 - 1], None)),
          ("packed", "a slice", (lg, torch.zeros((4, 2 * W8), dtype=torch.uint32)[:, :W8], None)),
          ("packed", "1-D", (lg, out.reshape(-1), None)),
          ("packed", "cap 17 of 16 cells", (lg, torch.zeros((4, 1 + 17 * 5), dtype=torch.uint32), None)),
          ("index", "int64", (lg, out, idx.long())), ("index", "3 of 4", (lg, out, idx[:3])), ("index", "2-D", (lg, out, idx.reshape(2, 2))),
          ("index", "strided", (lg, out, torch.zeros(8, dtype=torch.int32)[::2])), ("index", "a list", (lg, out, [0, 1, 2, 3]))]
    g["evaluate_packed"] = [(f"evaluate_actions_packed: {m} {what}", m, lambda a=a: policy_head.evaluate_actions_packed(env, *a))
                            for m, what, a in ev]
    g["evaluate_packed"] += [
        ("evaluate_actions_packed: cpu tensors for a cuda env", "logits: on cpu",
         lambda: policy_head.evaluate_actions_packed(cuda, lg, out)),
        # rows * H*W >= 2^31, on tensors that take no memory
        ("evaluate_actions_packed: 2^31 cells", "2\\^31", lambda: policy_head.evaluate_actions_packed(
            big, torch.empty((n_big, 256 * 256, 78), device="meta"), torch.empty((n_big, 6), dtype=torch.uint32, device="meta"))),
    ]

    # -- DeviceVecEnv.unpack on a stand-in --------------------------------------------------------------------------
    meta = torch.device("meta")
    bigfake = fake(dims=big.dims, device=meta, _h=types.SimpleNamespace(S=4, H=256, W=256, C=27, K=79))
    g["unpack"] = [
        ("unpack: packed int32", "packed", lambda: DeviceVecEnv.unpack(fake(), out.to(torch.int32))),
        ("unpack: packed 1-D", "packed", lambda: DeviceVecEnv.unpack(fake(), out.reshape(-1))),
        ("unpack: packed without rows", "packed", lambda: DeviceVecEnv.unpack(fake(), out[:0])),
        ("unpack: index a list", "index", lambda: DeviceVecEnv.unpack(fake(), out, index=[0, 1])),
        ("unpack: index 2-D", "index", lambda: DeviceVecEnv.unpack(fake(), out, index=idx.reshape(2, 2))),
        ("unpack: index int64", "index", lambda: DeviceVecEnv.unpack(fake(), out, index=idx[:3].long())),
        ("unpack: masks_out of 3 rows", "masks_out", lambda: DeviceVecEnv.unpack(fake(), out, masks_out=mk[:3])),
        ("unpack: actions_out int64", "actions_out", lambda: DeviceVecEnv.unpack(fake(), out, actions_out=ac.long())),
        ("unpack: 2^31 cells", "2\\^31", lambda: DeviceVecEnv.unpack(bigfake, torch.empty((n_big, 6), dtype=torch.uint32, device="meta"))),
        ("unpack: 2^31 cells through an index", "2\\^31", lambda: DeviceVecEnv.unpack(
            bigfake, torch.empty((2, 6), dtype=torch.uint32, device="meta"), index=torch.empty(n_big, dtype=torch.int32, device="meta"))),
    ]

    # -- packed observation rows: obs_pack, DeviceVecEnv.pack_obs / unpack_obs / onehot_packed on a stand-in --------
    fixed = 1 + (27 - 5) * 1  # word 0 and the bitmaps of planes 5.. of a 4x4 map
    O8 = fixed + 2 * 8
    pk = torch.zeros((4, O8), dtype=torch.uint32)
    ob = torch.zeros((4, 27, 4, 4), dtype=torch.int32)
    g["obs_packed_words"] = [(f"obs_pack.packed_words: cap {bad!r}", "cap", lambda bad=bad: obs_pack.packed_words(env, bad))
                             for bad in (0, -1, 17, 2.0, True, "8")]
    g["pack_obs"] = [
        ("pack_obs: out int32", "out", lambda: DeviceVecEnv.pack_obs(fake(), pk.to(torch.int32))),
        ("pack_obs: out one word more", "out", lambda: DeviceVecEnv.pack_obs(fake(), torch.zeros((4, O8 + 1), dtype=torch.uint32))),
        ("pack_obs: out one word short of cap 1", "out", lambda: DeviceVecEnv.pack_obs(fake(), torch.zeros((4, fixed + 1), dtype=torch.uint32))),
        ("pack_obs: cap 9 for cap 8's words", "out", lambda: DeviceVecEnv.pack_obs(fake(), pk, cap=9)),
        ("pack_obs: cap 0", "cap", lambda: DeviceVecEnv.pack_obs(fake(), pk, cap=0)),
        ("pack_obs: out 3-D", "out", lambda: DeviceVecEnv.pack_obs(fake(), pk.reshape(2, 2, O8))),
        ("pack_obs: out numpy", "out", lambda: DeviceVecEnv.pack_obs(fake(), pk.numpy())),
        ("pack_obs: out on another device", "out", lambda: DeviceVecEnv.pack_obs(fake(), torch.empty((4, O8), dtype=torch.uint32, device="meta"))),
        ("pack_obs: obs of 3 rows", "obs", lambda: DeviceVecEnv.pack_obs(fake(), pk, obs=ob[:3])),
        ("pack_obs: obs int64", "obs", lambda: DeviceVecEnv.pack_obs(fake(), pk, obs=ob.long())),
        ("pack_obs: obs permuted", "obs", lambda: DeviceVecEnv.pack_obs(fake(), pk, obs=ob.permute(0, 1, 3, 2))),
        ("pack_obs: 2^31 cells", "2\\^31", lambda: DeviceVecEnv.pack_obs(
            bigfake, torch.empty((n_big, 1 + 2 * 2 + 22 * 2048), dtype=torch.uint32, device="meta"),
            obs=torch.empty((n_big, 27, 256, 256), dtype=torch.int32, device="meta"))),
    ]
    g["read_obs"] = []
    for rname, read in (("unpack_obs", DeviceVecEnv.unpack_obs), ("onehot_packed", DeviceVecEnv.onehot_packed)):
        g["read_obs"] += [
            (f"{rname}: packed int32", "packed", lambda read=read: read(fake(), pk.to(torch.int32))),
            (f"{rname}: packed strided", "packed", lambda read=read: read(fake(), torch.zeros((4, 2 * O8), dtype=torch.uint32)[:, :O8])),
            (f"{rname}: packed without rows", "packed", lambda read=read: read(fake(), pk[:0])),
            (f"{rname}: packed 1-D", "packed", lambda read=read: read(fake(), pk.reshape(-1))),
            (f"{rname}: index int64", "index", lambda read=read: read(fake(), pk, index=idx[:3].long())),
            (f"{rname}: index 2-D", "index", lambda read=read: read(fake(), pk, index=idx.reshape(2, 2))),
            (f"{rname}: index a list", "index", lambda read=read: read(fake(), pk, index=[0, 1])),
            (f"{rname}: index on another device", "index", lambda read=read: read(fake(), pk, index=torch.empty(3, dtype=torch.int32, device="meta"))),
            (f"{rname}: 2^31 cells", "packed: rows", lambda read=read: read(
                bigfake, torch.empty((n_big, 1 + 2 * 2 + 22 * 2048), dtype=torch.uint32, device="meta"))),
            (f"{rname}: 2^31 cells through an index", "index: rows", lambda read=read: read(
                bigfake, torch.empty((2, 1 + 2 * 2 + 22 * 2048), dtype=torch.uint32, device="meta"),
                index=torch.empty(n_big, dtype=torch.int32, device="meta"))),
        ]
    g["read_obs"].append(("unpack_obs: out float32", "out",
                          lambda: DeviceVecEnv.unpack_obs(fake(), pk, out=torch.zeros((4, 27, 4, 4), dtype=torch.float32))))
    return g


def answer(call):
    """[exception type's name, full text] of a case's call"""
    try:
        call()
    except Exception as e:  # noqa: BLE001 (the type is what is recorded)
        return [type(e).__name__, str(e)]
    raise AssertionError("a refusal case raised nothing")


def answers():
    """name -> answer of every case, in order"""
    out = {}
    for group in cases().values():
        for name, _, call in group:
            assert name not in out, f"two cases named {name!r}"
            out[name] = answer(call)
    return out


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        json.dump(answers(), f, indent=1)
        f.write("\n")
