"""The masked policy head on the GPU (mrts_policy_head_*_dev, DeviceVecEnv.sample_actions, evaluate_actions)
against the float64 reference and numpy Philox of tests/policy_head_ref.py.

Shapes: 4x4 (16 cells: less than a wave), 9x8 (72 cells: a tail past 64), basesWorkers16x16 (the workload's).
Tables: the built-in one (K = 79) on every shape; tests/table_cases.py's r3, r5, t5r3 and t8r5 (K = 39, 55, 37, 56:
attack fields of 9 and 25 logits that leave most lanes of the field empty, 5 and 8 produce types that move every
later logit) on 4x4 and 9x8, as cases "4x4-r3" ...  nt and K come from the handle.
Masks: the environment's after 50 random steps (with its source bits), and synthetic ones (a slot without a
candidate, a slot with every bit of every cell set, empty / single-bit / scattered fields, scattered attack windows).

Tolerances are measured, not guessed: the same quantities computed by the reference in float32 on the CPU deviate
from the float64 reference by some largest amount over a test's inputs, and the kernels (which sum in another
order) get 4x that; the tests print both figures (MEASURED below records a run)."""
import math

import numpy as np
import pytest

from tests import policy_head_ref as R, table_cases as TC
from tests.defs import SEED
from tests.gpu_support import assert_same_outputs, ptr, torch_gpu

pytestmark = pytest.mark.gpu

MAPS = {"4x4": "maps/4x4/basesWorkers4x4.xml", "9x8": "maps/NoWhereToRun9x8.xml", "16x16": "maps/16x16/basesWorkers16x16.xml"}
S = 6
HSEED, HSTEP = 0x0123456789ABCDEF, 17
# x the fp32 CPU reference's largest deviation from the float64 reference over a test's inputs (_bound).
# MEASURED on an MI355X (fp32 CPU reference's deviation -> bound; the kernels' deviation):
#   log-probability / entropy  4x4: 1.2e-5 -> 4.9e-5; 5.6e-6    9x8: 5.5e-5 -> 2.2e-4; 2.2e-5    16x16: 1.7e-4 -> 6.7e-4; 8.0e-5
#   gradient                   4x4: 7.2e-7 -> 2.9e-6; 7.2e-7    9x8: 1.3e-6 -> 5.1e-6; 7.2e-7    16x16: 1.3e-6 -> 5.2e-6; 7.2e-7
# the tables of tests/table_cases.py, the same three figures, 4x4 then 9x8:
#   log-probability / entropy  r5:   1.2e-5 -> 4.9e-5; 5.9e-6    5.6e-5 -> 2.2e-4; 2.0e-5
#                              r3:   7.7e-6 -> 3.1e-5; 5.2e-6    5.3e-5 -> 2.1e-4; 2.1e-5
#                              t5r3: 8.8e-6 -> 3.5e-5; 5.2e-6    5.2e-5 -> 2.1e-4; 2.1e-5
#                              t8r5: 1.3e-5 -> 5.1e-5; 4.6e-6    5.5e-5 -> 2.2e-4; 2.2e-5
#   gradient                   r5:   4.2e-7 -> 1.7e-6; 5.1e-7    7.2e-7 -> 2.9e-6; 4.8e-7
#                              r3:   4.8e-7 -> 1.9e-6; 7.2e-7    4.8e-7 -> 1.9e-6; 3.6e-7
#                              t5r3: 4.2e-7 -> 1.7e-6; 3.6e-7    4.8e-7 -> 1.9e-6; 4.8e-7
#                              t8r5: 7.7e-7 -> 3.1e-6; 4.2e-7    6.6e-7 -> 2.6e-6; 4.8e-7
# (the sums run over up to 256 cells x 7 fields, magnitude ~3e3 in the every-bit-set rows; the kernels keep their
# per-lane partial sums in double — with fp32 partial sums the 16x16 figure was 3.5e-4)
TOL_FACTOR = 4.0


def _sample(env, logits, masks, source, seed, step):
    """the C entry on any masks / source bits: (actions, logprob, entropy)"""
    torch = torch_gpu()
    from microrts_amd import _lib

    n = env._h.S
    out = torch.full((n, logits.shape[1], 7), -7, dtype=torch.int32, device=env.device)
    lp, ent = (torch.full((n,), math.nan, dtype=torch.float32, device=env.device) for _ in range(2))
    _lib.check(env._h.L.mrts_policy_head_sample_dev(env._h.h, ptr(logits), ptr(masks), ptr(source), seed, step, ptr(out), ptr(lp),
                                                    ptr(ent), env._s(None)))
    return out, lp, ent


CASES = list(MAPS) + [f"{shape}-{t}" for t in TC.IDS for shape in ("4x4", "9x8")]


class Case:
    """one shape and table ("9x8", "9x8-r5"): an env stepped 50 times, its masks / source bits, synthetic masks,
    logits, the float64 reference"""

    def __init__(self, name):
        torch = torch_gpu()
        from microrts_amd import DeviceVecEnv, UnitTypeTable

        shape, _, table = name.partition("-")
        utt = UnitTypeTable.fromJSON(TC.utt_json(table)) if table else UnitTypeTable()
        self.env = env = DeviceVecEnv(S, 0, 2000, [MAPS[shape]] * S, seed=3, utt=utt)
        env.reset()
        for k in range(50):
            env.random_policy(SEED, k)
            env.step()
        _, H, W, _, K = env.dims
        # the handle's own type count: its one-hot observation has 5 + 5 + 3 + (nt + 1) + 6 + 2 features
        self.HW, self.K, self.nt = H * W, K, env._h.L.mrts_onehot_features(env._h.h) - 22
        assert (self.nt, K) == ((TC.TABLES[table].nt, TC.TABLES[table].K) if table else (7, 79))
        assert not (table and env.multi_step_capable), "only the K = 79 instances run several steps per launch"
        assert K == 23 + self.nt + (2 * utt.getMaxAttackRange() + 1) ** 2
        g = torch.Generator().manual_seed(H * W)
        self.logits_cpu = 3 * torch.randn((S, H * W, K - 1), generator=g)
        self.logits = self.logits_cpu.to(env.device)
        syn = R.synthetic_masks(S, H * W, K, self.nt, seed=H * W)
        self.masks = {"env": env.masks.clone().reshape(S, H * W, K), "syn": torch.from_numpy(syn).to(env.device)}
        self.source = {"env": env.source.clone(), "syn": torch.from_numpy(R.source_bits(syn)).to(env.device)}
        assert np.array_equal(R.source_bits(self.masks["env"].cpu().numpy()), self.source["env"].cpu().numpy())
        self.u = torch.from_numpy(np.stack([R.head_uniforms(HSEED, s, HSTEP, H * W) for s in range(S)]))
        self._ref = {}

    def ref(self, kind):
        if kind not in self._ref:
            self._ref[kind] = R.head_reference(self.logits_cpu, self.masks[kind].cpu(), self.nt, u=self.u)
        return self._ref[kind]


_CASES = {}


def _case(shape):
    if shape not in _CASES:
        _CASES[shape] = Case(shape)
    return _CASES[shape]


@pytest.fixture(scope="module", autouse=True)
def _close_table_cases():
    """the table cases' handles end with the module; the three built-in ones stay, as before"""
    yield
    for name in [n for n in _CASES if "-" in n]:
        _CASES.pop(name).env.close()


@pytest.fixture(params=CASES)
def case(request):
    return _case(request.param)


def _bound(name, torch, pairs):
    """4 x the largest deviation of the fp32 CPU reference from the float64 one over (fp32, fp64) tensor pairs"""
    dev = max(float((a.double() - b).abs().max()) for a, b in pairs)
    print(f"{name}: fp32 CPU reference deviates by {dev:.3e}; bound {TOL_FACTOR * dev:.3e}")
    assert dev > 0
    return TOL_FACTOR * dev


@pytest.mark.parametrize("kind", ["env", "syn"])
def test_legality_zero_rows_and_both_candidate_forms(case, kind):
    torch = torch_gpu()
    env, m = case.env, case.masks[kind]
    a, lp, ent = _sample(env, case.logits, m, case.source[kind], HSEED, HSTEP)
    a2, lp2, ent2 = _sample(env, case.logits, m, None, HSEED, HSTEP)
    assert torch.equal(a, a2) and torch.equal(lp, lp2) and torch.equal(ent, ent2), "source bits vs mask byte 0"
    a, mc = a.cpu().long(), m.cpu() != 0
    cand = mc[..., 0]
    assert kind == "env" or (not cand[0].any() and cand[1].all())
    assert cand.any() and (a[~cand] == 0).all(), "rows of cells that are no candidates"
    for f, (lo, hi) in enumerate(R.fields(case.K, case.nt)):
        bits = mc[..., 1 + lo:1 + hi] & cand[..., None]
        comp = a[..., f]
        assert ((comp >= 0) & (comp < hi - lo)).all(), f"field {f}: component out of range"
        on = torch.gather(bits, -1, comp[..., None])[..., 0]
        ne = bits.any(-1)
        assert on[ne].all(), f"field {f}: a component off the mask"
        assert (comp[~ne] == 0).all(), f"field {f}: an empty field's component is not 0"
    if kind == "env":  # the environment accepts the rows (it ignores the parameters of other types)
        assert torch.equal(env.masks.reshape(m.shape), m)
        acts, lp3, _ = env.sample_actions(case.logits, HSEED, HSTEP)
        assert acts is env.actions and torch.equal(acts.cpu().long(), a) and torch.equal(lp3, lp)
        env.step()
        assert not env.error_flags().any()


@pytest.mark.parametrize("kind", ["env", "syn"])
def test_draws_equal_the_float64_reference(case, kind):
    a, _, _ = _sample(case.env, case.logits, case.masks[kind], case.source[kind], HSEED, HSTEP)
    r = case.ref(kind)
    drawn, near = int(r["drawn"].sum()), int(r["near"].sum())
    print(f"{kind}: {drawn} drawn components, {near} within 1e-5 of a boundary")
    assert drawn > 0 and near <= 0.01 * drawn
    keep = r["drawn"] & ~r["near"]
    a = a.cpu().long()
    assert (a[keep] == r["actions"][keep]).all(), f"{int((a[keep] != r['actions'][keep]).sum())} draws differ"
    assert (a[~r["drawn"]] == 0).all()


def test_stream_identity():
    """slot 0 of a handle with slot_id_base 3 draws what slot 3 of a base-0 handle draws; step and seed matter"""
    torch = torch_gpu()
    from microrts_amd import DeviceVecEnv

    c = _case("9x8")
    m, src = c.masks["syn"], c.source["syn"]
    a, lp, ent = _sample(c.env, c.logits, m, src, HSEED, HSTEP)
    B = DeviceVecEnv(S, 0, 2000, [MAPS["9x8"]] * S, seed=3, slot_id_base=3)
    roll = lambda t: torch.roll(t, -3, 0).contiguous()
    b, lpb, entb = _sample(B, roll(c.logits), roll(m), roll(src), HSEED, HSTEP)
    for s in range(S - 3):  # B's slot s has id 3 + s and A's row 3 + s
        assert torch.equal(b[s], a[3 + s]) and lpb[s] == lp[3 + s] and entb[s] == ent[3 + s]
    assert not torch.equal(b[3:], a[:3]), "rows 0..2 under ids 6..8 drew what ids 0..2 drew"
    B.close()
    for seed, step in ((HSEED, HSTEP + 1), (HSEED + 1, HSTEP)):
        assert not torch.equal(_sample(c.env, c.logits, m, src, seed, step)[0], a)


def test_frequencies():
    """one candidate cell, type bits 1 2 4 with logits log 1, log 2, log 5, over 4096 steps: counts within 5 sigma"""
    torch = torch_gpu()
    c = _case("4x4")
    env = c.env
    masks = torch.zeros((S, c.HW, c.K), dtype=torch.uint8, device=env.device)
    logits = torch.full((S, c.HW, c.K - 1), math.nan, device=env.device)
    masks[0, 5, 0] = 1
    for j, v in ((1, 1.0), (2, 2.0), (4, 5.0)):
        masks[0, 5, 1 + j] = 1
        logits[0, 5, j] = math.log(v)
    src = torch.from_numpy(R.source_bits(masks.cpu().numpy())).to(env.device)
    n = 4096
    outs = torch.zeros((n, S, c.HW, 7), dtype=torch.int32, device=env.device)
    L = env._h.L
    for t in range(n):
        assert L.mrts_policy_head_sample_dev(env._h.h, ptr(logits), ptr(masks), ptr(src), 99, t, ptr(outs[t]), None, None,
                                             env._s(None)) == 0
    got = outs[:, 0, 5, 0].cpu().numpy()
    assert outs.sum().item() == got.sum()
    for j, p in ((1, 1 / 8), (2, 2 / 8), (4, 5 / 8)):
        k, sigma = int((got == j).sum()), math.sqrt(n * p * (1 - p))
        print(f"type {j}: {k} of {n}, expected {n * p:.0f} +- {sigma:.1f}")
        assert abs(k - n * p) <= 5 * sigma
    assert np.isin(got, (1, 2, 4)).all()


def _score(env, logits, masks, actions):
    torch = torch_gpu()
    from microrts_amd import _lib

    n = logits.shape[0]
    lp, ent = (torch.full((n,), math.nan, dtype=torch.float32, device=env.device) for _ in range(2))
    _lib.check(env._h.L.mrts_policy_head_score_dev(env._h.h, n, ptr(logits), ptr(masks), ptr(actions), ptr(lp), ptr(ent), env._s(None)))
    return lp, ent


def _rows(c, n, seed):
    """n rows of logits / synthetic masks / on-mask actions (drawn by the reference from numpy uniforms)"""
    torch = torch_gpu()
    g = torch.Generator().manual_seed(seed)
    logits = 3 * torch.randn((n, c.HW, c.K - 1), generator=g)
    masks = torch.from_numpy(R.synthetic_masks(n, c.HW, c.K, c.nt, seed=seed))
    u = torch.rand((n, c.HW, 7), generator=g, dtype=torch.float64)
    acts = R.head_reference(logits, masks, c.nt, u=u)["actions"].to(torch.int32)
    return logits, masks, acts


def test_logprob_and_entropy(case):
    torch = torch_gpu()
    env, dev = case.env, case.env.device
    runs = []  # (kernel logprob, kernel entropy, float32 reference, float64 reference)
    for kind in ("env", "syn"):
        a, lp, ent = _sample(env, case.logits, case.masks[kind], case.source[kind], HSEED, HSTEP)
        lps, ents = _score(env, case.logits, case.masks[kind], a)
        assert torch.equal(lp, lps) and torch.equal(ent, ents), f"{kind}: sample and score differ in a bit"
        args = (case.logits_cpu, case.masks[kind].cpu(), case.nt)
        runs.append((lp, ent, R.head_reference(*args, actions=a.cpu(), dtype=torch.float32), R.head_reference(*args, actions=a.cpu())))
    for n in (1, 3, 130):
        logits, masks, acts = _rows(case, n, seed=1000 + n)
        lp, ent = _score(env, logits.to(dev), masks.to(dev), acts.to(dev))
        runs.append((lp, ent, R.head_reference(logits, masks, case.nt, actions=acts, dtype=torch.float32),
                     R.head_reference(logits, masks, case.nt, actions=acts)))
    tol = _bound("logprob / entropy", torch, [(r32[k], r64[k]) for _, _, r32, r64 in runs for k in ("logprob", "entropy")])
    worst = 0.0
    for lp, ent, _, r64 in runs:
        assert torch.isfinite(lp).all() and torch.isfinite(ent).all()
        worst = max(worst, float((lp.cpu().double() - r64["logprob"]).abs().max()), float((ent.cpu().double() - r64["entropy"]).abs().max()))
    print(f"kernels deviate from the float64 reference by {worst:.3e}")
    assert worst <= tol


def test_exact_logprob_cases(case):
    torch = torch_gpu()
    env, dev = case.env, case.env.device
    masks = torch.zeros((3, case.HW, case.K), dtype=torch.uint8)
    masks[0, :, 1:] = 1  # row 0: no candidate
    cell = case.HW - 1  # rows 1, 2: one candidate, a single-bit type field and a single-bit attack window
    for r in (1, 2):
        masks[r, cell, 0] = masks[r, cell, 1 + 5] = masks[r, cell, case.K - 1] = 1
    acts = torch.zeros((3, case.HW, 7), dtype=torch.int32)
    acts[1:, cell, 0], acts[1:, cell, 6] = 5, case.K - 2 - (22 + case.nt)
    acts[2, cell, 6] -= 1  # row 2: the attack index is off the mask
    logits = 3 * torch.randn((3, case.HW, case.K - 1), generator=torch.Generator().manual_seed(5))
    lp, ent = _score(env, logits.to(dev), masks.to(dev), acts.to(dev))
    assert lp.tolist() == [0.0, 0.0, -math.inf] and ent.tolist() == [0.0, 0.0, 0.0]
    acts[2, cell, 6] = 1000  # outside the field altogether
    assert _score(env, logits.to(dev), masks.to(dev), acts.to(dev))[0].tolist() == [0.0, 0.0, -math.inf]


def _grad(env, logits, masks, acts, g_lp, g_ent):
    torch = torch_gpu()
    from microrts_amd import _lib

    out = torch.full_like(logits, math.nan)  # garbage: every element must be overwritten
    _lib.check(env._h.L.mrts_policy_head_grad_dev(env._h.h, logits.shape[0], ptr(logits), ptr(masks), ptr(acts), ptr(g_lp), ptr(g_ent),
                                                  ptr(out), env._s(None)))
    return out


def test_masked_logits_are_never_read(case):
    torch = torch_gpu()
    env, dev = case.env, case.env.device
    for kind in ("env", "syn"):
        m = case.masks[kind]
        setbit = (m[..., 1:] != 0) & (m[..., :1] != 0)
        poison = torch.where(torch.arange(case.K - 1, device=dev) % 2 == 0, math.nan, math.inf).expand_as(case.logits)
        bad = torch.where(setbit, case.logits, poison).contiguous()
        g = torch.rand((2, S), generator=torch.Generator().manual_seed(3)).to(dev)
        for src in (case.source[kind], None):
            a, lp, ent = _sample(env, case.logits, m, src, HSEED, HSTEP)
            ab, lpb, entb = _sample(env, bad, m, src, HSEED, HSTEP)
            assert torch.equal(a, ab) and torch.equal(lp, lpb) and torch.equal(ent, entb)
            assert torch.isfinite(lp).all() and torch.isfinite(ent).all()
        lps, ents = _score(env, bad, m, a)
        assert torch.equal(lps, lp) and torch.equal(ents, ent)
        gr, grb = _grad(env, case.logits, m, a, g[0], g[1]), _grad(env, bad, m, a, g[0], g[1])
        assert torch.equal(gr, grb) and torch.isfinite(gr).all()
        # set-bit logits of +-80: the maximum is subtracted before the exponential
        big = torch.where(torch.rand(case.logits.shape, generator=torch.Generator().manual_seed(4)).to(dev) < 0.5, 80.0, -80.0)
        a, lp, ent = _sample(env, big, m, case.source[kind], HSEED, HSTEP)
        assert torch.isfinite(lp).all() and torch.isfinite(ent).all() and torch.isfinite(_grad(env, big, m, a, g[0], g[1])).all()


def test_gradient(case):
    torch = torch_gpu()
    from microrts_amd import evaluate_actions

    env, dev = case.env, case.env.device
    worst, pairs = 0.0, []
    for n in (1, 3, 130):
        logits, masks, acts = _rows(case, n, seed=2000 + n)
        if n == 3:  # a component off its field's mask: that field keeps only its entropy term
            cand = (masks[2, :, 0] != 0).nonzero()[0, 0]
            masks[2, cand, 1:7] = torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.uint8)
            acts[2, cand, 0] = 1
        gen = torch.Generator().manual_seed(n)
        g_lp, g_ent = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
        refs = []
        for dtype in (torch.float32, torch.float64):
            x = logits.clone().requires_grad_(True)
            r = R.head_reference(x, masks, case.nt, actions=acts, dtype=dtype)
            # (a row with a component off its mask has logprob -inf, so the loss is not finite; its gradient is)
            ((r["logprob"] * g_lp.to(dtype)).sum() + (r["entropy"] * g_ent.to(dtype)).sum()).backward()
            refs.append(x.grad)
        pairs.append((refs[0], refs[1].double()))
        x = logits.to(dev).requires_grad_(True)
        md, ad = masks.to(dev), acts.to(dev)
        lp, ent = evaluate_actions(env, x, md.reshape(n, *env.dims[1:3], case.K), ad)
        assert lp.requires_grad and ent.requires_grad
        assert torch.equal(torch.isfinite(lp).cpu(), torch.tensor([not (n == 3 and r == 2) for r in range(n)]))
        ((lp * g_lp.to(dev)).sum() + (ent * g_ent.to(dev)).sum()).backward()
        gk = x.grad
        assert torch.equal(gk, _grad(env, x.detach(), md, ad, g_lp.to(dev), g_ent.to(dev))), "autograd path vs the C entry"
        dead = ~(((masks[..., 1:] != 0) & (masks[..., :1] != 0)).to(dev))
        assert (gk[dead] == 0).all(), "gradient at cleared bits / cells that are no candidates"
        worst = max(worst, float((gk.cpu().double() - refs[1].double()).abs().max()))
        # the log-probability alone (no entropy gradient), logits the only input that requires grad
        x2 = logits.to(dev).requires_grad_(True)
        lp2, _ = evaluate_actions(env, x2, md, ad)
        (lp2 * g_lp.to(dev)).sum().backward()
        assert torch.equal(x2.grad, _grad(env, x2.detach(), md, ad, g_lp.to(dev), None))
    tol = _bound("gradient", torch, pairs)
    print(f"kernel gradient deviates from the float64 reference by {worst:.3e}")
    assert worst <= tol


def test_determinism_and_bookkeeping():
    torch = torch_gpu()
    from microrts_amd import DeviceVecEnv, _lib

    c = _case("16x16")
    for kind in ("env", "syn"):
        one = _sample(c.env, c.logits, c.masks[kind], c.source[kind], HSEED, HSTEP)
        two = _sample(c.env, c.logits, c.masks[kind], c.source[kind], HSEED, HSTEP)
        assert all(torch.equal(x, y) for x, y in zip(one, two))
        g = torch.ones(S, device=c.env.device)
        assert torch.equal(_grad(c.env, c.logits, c.masks[kind], one[0], g, g), _grad(c.env, c.logits, c.masks[kind], one[0], g, g))
    # A samples into env.actions between fused / policy calls; B (a fresh handle) replays the same rows written by
    # torch, followed by an explicit mrts_policy_invalidate
    A, B = (DeviceVecEnv(S, 0, 2000, [MAPS["16x16"]] * S, seed=3) for _ in range(2))

    def head(step):
        acts, _, _ = A.sample_actions(c.logits, HSEED, step)
        assert acts is A.actions
        B.actions.copy_(A.actions)
        _lib.check(B._h.L.mrts_policy_invalidate(B._h.h))

    for e in (A, B):
        e.reset()
        e.random_policy(SEED, 0)
        for k in range(1, 6):
            e.step_fused(SEED, k)
    assert_same_outputs(A, B, "fused warm-up")
    head(5)
    for e in (A, B):
        e.step_fused(SEED, 6)
    assert_same_outputs(A, B, "step_fused after sample_actions")
    head(6)
    for e in (A, B):
        e.random_policy(SEED, 7)
    assert_same_outputs(A, B, "random_policy after sample_actions")
    for e in (A, B):
        e.step()
        e.random_policy(SEED, 8)
    head(8)
    for e in (A, B):
        e.step()
    assert_same_outputs(A, B, "step after sample_actions")
    head(9)
    for e in (A, B):
        e.rollout_fused(SEED, 10, 6)
    assert_same_outputs(A, B, "rollout_fused after sample_actions")
    A.close()
    B.close()


def test_refusals():
    torch = torch_gpu()
    from microrts_amd import ForwardModel, JNIGridnetVecClient, _lib

    m = MAPS["4x4"]
    bots = JNIGridnetVecClient.bots(100, None, "", [m] * 2, ["PassiveAI"] * 2, ["PassiveAI"] * 2)
    fm = ForwardModel(2, m, policies=("PassiveAI", "PassiveAI"))
    dev = torch.device("cuda", 0)
    lg = torch.zeros((2, 16, 78), device=dev)
    mk = torch.zeros((2, 16, 79), dtype=torch.uint8, device=dev)
    ac = torch.zeros((2, 16, 7), dtype=torch.int32, device=dev)
    L = _lib.load()
    for h in (bots._h, fm._h):
        calls = [L.mrts_policy_head_sample_dev(h.h, ptr(lg), ptr(mk), None, 1, 0, ptr(ac), None, None, None),
                 L.mrts_policy_head_score_dev(h.h, 2, ptr(lg), ptr(mk), ptr(ac), None, None, None),
                 L.mrts_policy_head_grad_dev(h.h, 2, ptr(lg), ptr(mk), ptr(ac), None, None, ptr(lg.clone()), None)]
        for rc in calls:
            assert rc == -95 and "bot-only or forward-model" in L.mrts_last_error().decode()  # -ENOTSUP
    bots.close()
    fm.close()
    env = _case("4x4").env
    h = env._h
    assert L.mrts_policy_head_score_dev(h.h, -1, ptr(lg), ptr(mk), ptr(ac), None, None, None) == -22  # -EINVAL
    assert L.mrts_policy_head_score_dev(h.h, (1 << 31) // 16, ptr(lg), ptr(mk), ptr(ac), None, None, None) == -22
    assert L.mrts_policy_head_score_dev(h.h, 2, None, ptr(mk), ptr(ac), None, None, None) == -22
    assert L.mrts_policy_head_grad_dev(h.h, 2, ptr(lg), ptr(mk), ptr(ac), None, None, None, None) == -22
    assert L.mrts_policy_head_sample_dev(h.h, ptr(lg), None, None, 1, 0, ptr(ac), None, None, None) == -22
    with pytest.raises(ValueError, match="logits"):
        env.sample_actions(torch.zeros((S, 16, 78), dtype=torch.float64, device=dev), 1, 0)
    with pytest.raises(ValueError, match="out"):
        env.sample_actions(torch.zeros((S, 16, 78), device=dev), 1, 0, out=torch.zeros((S, 16, 7), device=dev))
