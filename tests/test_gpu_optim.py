"""The fused trainer's update rules on the device: the kernels of csrc/optim.hip through the raw C ABI on guarded buffers, then
``SegTrainer(..., optimizer=, clip_grad_norm=)`` and the plain trainer, which takes the same path: rules, metadata, state dicts /
checkpoints, two data-parallel ranks.

Every comparison is one step of the fp64 restatement of tests/optim_cases.py from the device's own pre-step fp32 state, within the
bound derived there (roundings of the expression x 2^-24 x the magnitudes they act on); bit-equalities are bit-equalities."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import optim_cases as OC
from flair_amd import optim as FO

pytestmark = pytest.mark.gpu

GUARD = 256
LR = 0.05
CASES = OC.rule_cases()


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 4: torch.int32, 8: torch.int64}[t.element_size()])


class _Guarded:
    """n elements inside an allocation of n + 2 * GUARD elements filled with ``fill`` (as tests/test_gpu_tta.py keeps its outputs)"""

    def __init__(self, dev, n, dtype, fill, data=None):
        self.n = n
        self.full = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
        if data is not None:
            self.full[GUARD:GUARD + n] = torch.as_tensor(data, dtype=dtype).to(dev)
        self.before = _bits(self.full.cpu().clone())
        self.ptr = self.full.data_ptr() + GUARD * self.full.element_size()

    def read(self, what):
        after = self.full.cpu()
        a = _bits(after)
        assert torch.equal(a[:GUARD], self.before[:GUARD]), f"{what}: written before the buffer"
        assert torch.equal(a[GUARD + self.n:], self.before[GUARD + self.n:]), f"{what}: written behind the buffer"
        return after[GUARD:GUARD + self.n]

    def unchanged(self, what):
        assert torch.equal(_bits(self.full.cpu()), self.before), f"{what} was written"


def _lib():
    from flair_amd import _lib as L
    return L, L.lib()


def _sgd(lib, L, p, g, buf, n, lr, hp, first, gs=1.0, coef=None):
    return lib.flair_optim_sgd(p, g, buf, n, lr, hp["momentum"], hp["dampening"], hp["weight_decay"], int(hp["nesterov"]), int(first), gs,
                               coef, L.stream())


def _adamw(lib, L, p, g, m, v, n, lr, hp, t, first, gs=1.0, coef=None):
    bc1, bc2 = OC.bias_corrections(hp["betas"], t)
    return lib.flair_optim_adamw(p, g, m, v, n, lr, hp["betas"][0], hp["betas"][1], hp["eps"], hp["weight_decay"], bc1, bc2, int(first),
                                 gs, coef, L.stream())


# ------------------------------------------------------------------------------------------------------------------ the rules
@pytest.fixture(scope="module")
def inputs():
    """One set of fp32 inputs per size, shared and never written: (p0, [g of step 0, 1, 2])"""
    out = {}
    for n in OC.SIZES:
        g = OC.rand_f32(n, 100 + n % 97, scale=0.1)
        out[n] = (OC.rand_f32(n, n % 89), [g, (g * np.float32(-1.5)).astype(np.float32), np.roll(g, 1)])
    return out


@pytest.mark.parametrize("n", OC.SIZES)
@pytest.mark.parametrize("case", CASES, ids=OC.case_id)
def test_rules_three_steps_within_the_bound(dev, inputs, n, case):
    """State starts NaN-filled: the first step may not read it.  grads stay bit-unchanged, the guards intact."""
    L, lib = _lib()
    kind, hp, scaled = case
    p0, grads = inputs[n]
    p = _Guarded(dev, n, torch.float32, 7.0, p0)
    s1 = _Guarded(dev, n, torch.float32, float("nan"))
    s2 = _Guarded(dev, n, torch.float32, float("nan"))
    gs = 0.5 if scaled else 1.0
    coef_t = torch.tensor([0.625], dtype=torch.float32, device=dev) if scaled else None
    coef, coef_v = (coef_t.data_ptr(), 0.625) if scaled else (None, None)
    lr = LR if kind == "sgd" else 1e-3
    for step in range(3):
        g = _Guarded(dev, n, torch.float32, 3.0, grads[step])
        pre_p, pre_1, pre_2 = p.read("p").numpy().copy(), s1.read("state 1").numpy().copy(), s2.read("state 2").numpy().copy()
        first = step == 0
        if kind == "sgd":
            rc = _sgd(lib, L, p.ptr, g.ptr, s1.ptr if hp["momentum"] else None, n, lr, hp, first, gs, coef)
        else:
            rc = _adamw(lib, L, p.ptr, g.ptr, s1.ptr, s2.ptr, n, lr, hp, step + 1, first, gs, coef)
        assert rc == 0, rc
        torch.cuda.synchronize()
        g.unchanged("grads")
        got_p = p.read("p").numpy()
        if kind == "sgd":
            want_p, want_b, bp, bb = OC.sgd_step64(pre_p, grads[step], pre_1, lr, hp, first, gs, coef_v)
            ok, worst = OC.within(got_p, want_p, bp)
            assert ok, (step, "p", worst)
            if hp["momentum"]:
                ok, worst = OC.within(s1.read("buf").numpy(), want_b, bb)
                assert ok, (step, "buf", worst)
            else:
                s1.unchanged("momentum buffer without momentum")
            s2.unchanged("second state of SGD")
        else:
            want_p, want_m, want_v, bp, bm, bv = OC.adamw_step64(pre_p, grads[step], pre_1, pre_2, lr, hp, step + 1, first, gs, coef_v)
            for name, got, want, b in (("p", got_p, want_p, bp), ("m", s1.read("m").numpy(), want_m, bm), ("v", s2.read("v").numpy(), want_v, bv)):
                ok, worst = OC.within(got, want, b)
                assert ok, (step, name, worst)
        assert np.isfinite(got_p).all()
    assert not np.array_equal(got_p, p0)


@pytest.mark.parametrize("n", OC.SIZES)
def test_default_sgd_is_flair_sgd_step_to_the_bit(dev, inputs, n):
    L, lib = _lib()
    p0, grads = inputs[n]
    a, b = _Guarded(dev, n, torch.float32, 7.0, p0), _Guarded(dev, n, torch.float32, 7.0, p0)
    g = _Guarded(dev, n, torch.float32, 3.0, grads[0])
    hp = dict(momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False)
    for _ in range(2):
        assert _sgd(lib, L, a.ptr, g.ptr, None, n, LR, hp, first=False) == 0
        assert lib.flair_sgd_step(b.ptr, g.ptr, n, LR, L.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(a.read("optim_sgd")), _bits(b.read("sgd_step")))
    assert not torch.equal(_bits(a.read("optim_sgd")), _bits(torch.from_numpy(p0)))


def test_first_steps_ignore_nan_state_and_later_steps_read_it(dev, inputs):
    L, lib = _lib()
    n = 1028
    p0, grads = inputs[n]
    g = _Guarded(dev, n, torch.float32, 3.0, grads[0])
    hp = dict(momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=False)
    ahp = OC.adamw_grid()[1]
    for first, finite in ((True, True), (False, False)):
        p, buf = _Guarded(dev, n, torch.float32, 7.0, p0), _Guarded(dev, n, torch.float32, float("nan"))
        assert _sgd(lib, L, p.ptr, g.ptr, buf.ptr, n, LR, hp, first=first) == 0
        q, m, v = _Guarded(dev, n, torch.float32, 7.0, p0), _Guarded(dev, n, torch.float32, float("nan")), _Guarded(dev, n, torch.float32, float("nan"))
        assert _adamw(lib, L, q.ptr, g.ptr, m.ptr, v.ptr, n, 1e-3, ahp, 1, first=first) == 0
        torch.cuda.synchronize()
        for t in (p, buf, q, m, v):
            assert bool(torch.isfinite(t.read("out")).all()) == finite


# ------------------------------------------------------------------------------------------------------------------ the norm
def _sqnorm(dev, arrays, repeat=1):
    """sum of squares over the arrays in turn (the accumulate flag from the second on): the fp64 device value, as a Python float"""
    L, lib = _lib()
    npart = lib.flair_grad_sqnorm_partials()
    partials = _Guarded(dev, npart, torch.float64, -1.0)
    out = _Guarded(dev, 1, torch.float64, float("nan"))
    vals = []
    for _ in range(repeat):
        for k, a in enumerate(arrays):
            g = _Guarded(dev, a.size, torch.float32, 3.0, a)
            assert lib.flair_grad_sqnorm(g.ptr, a.size, partials.ptr, out.ptr, int(k > 0), L.stream()) == 0
            torch.cuda.synchronize()
            g.unchanged("grads")
        partials.read("partials")
        vals.append(out.read("sum").clone())
    return vals


@pytest.mark.parametrize("n", OC.SIZES)
def test_sqnorm_exact_on_small_integers_and_repeatable(dev, n):
    rng = np.random.default_rng(n)
    a = rng.integers(-2, 3, n).astype(np.float32)
    one, two = _sqnorm(dev, [a], repeat=2)
    assert float(one) == float(np.sum(a.astype(np.float64) ** 2))
    assert torch.equal(_bits(one), _bits(two))


@pytest.mark.parametrize("n", OC.SIZES)
def test_sqnorm_random_within_2pow24_of_fp64_and_repeatable(dev, inputs, n):
    a = inputs[n][1][0]
    one, two = _sqnorm(dev, [a], repeat=2)
    want = np.sqrt(OC.sqnorm64(a))
    assert abs(np.sqrt(float(one)) - want) <= OC.U * want
    assert torch.equal(_bits(one), _bits(two))


@pytest.mark.parametrize("n", [7, 1028, OC.SIZES[-1]])
def test_sqnorm_two_buffers_equal_their_concatenation(dev, inputs, n):
    rng = np.random.default_rng(n + 1)
    a, b = rng.integers(-2, 3, n).astype(np.float32), rng.integers(-2, 3, 1031).astype(np.float32)
    (both,), (cat,) = _sqnorm(dev, [a, b]), _sqnorm(dev, [np.concatenate([a, b])])
    assert torch.equal(_bits(both), _bits(cat))   # integers: every partial sum is exact, any order gives these bits
    ra, rb = inputs[n][1][0], inputs[1028][1][1]
    (both,) = _sqnorm(dev, [ra, rb])
    want = np.sqrt(OC.sqnorm64(ra, rb))
    assert abs(np.sqrt(float(both)) - want) <= OC.U * want


# ------------------------------------------------------------------------------------------------------------------ the clip
def _clip(dev, sq, max_norm, gs=1.0):
    L, lib = _lib()
    s = _Guarded(dev, 1, torch.float64, 0.0, [sq])
    norm, coef = _Guarded(dev, 1, torch.float32, float("nan")), _Guarded(dev, 1, torch.float32, float("nan"))
    assert lib.flair_clip_coef(s.ptr, gs, max_norm, norm.ptr, coef.ptr, L.stream()) == 0
    torch.cuda.synchronize()
    s.unchanged("the sum")
    return norm, coef


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_clip_inactive_is_exactly_one_and_the_step_is_the_unclipped_one(dev, inputs, kind):
    L, lib = _lib()
    n = 1028
    p0, grads = inputs[n]
    sq = OC.sqnorm64(grads[0])
    norm, coef = _clip(dev, sq, max_norm=2 * float(np.sqrt(sq)))
    assert float(coef.read("coef")) == 1.0
    want_norm, _, bn, _ = OC.clip64(sq, 2 * float(np.sqrt(sq)))
    assert abs(float(norm.read("norm")) - float(want_norm)) <= bn
    hp = dict(momentum=0.9, dampening=0.0, weight_decay=1e-2, nesterov=True) if kind == "sgd" else OC.adamw_grid()[1]
    res = []
    for c in (coef.ptr, None):
        p, s1, s2 = (_Guarded(dev, n, torch.float32, 7.0, p0) for _ in range(3))
        g = _Guarded(dev, n, torch.float32, 3.0, grads[0])
        for step in range(2):
            if kind == "sgd":
                assert _sgd(lib, L, p.ptr, g.ptr, s1.ptr, n, LR, hp, step == 0, 1.0, c) == 0
            else:
                assert _adamw(lib, L, p.ptr, g.ptr, s1.ptr, s2.ptr, n, 1e-3, hp, step + 1, step == 0, 1.0, c) == 0
        torch.cuda.synchronize()
        res.append([_bits(t.read("out")) for t in (p, s1, s2)])
    assert all(torch.equal(a, b) for a, b in zip(*res))


@pytest.mark.parametrize("gs", [1.0, 0.5])
def test_clip_active_matches_the_restatement(dev, inputs, gs):
    L, lib = _lib()
    n = 1028
    p0, grads = inputs[n]
    (sq_t,) = _sqnorm(dev, [grads[0]])
    sq = float(sq_t)
    max_norm = 0.25 * float(np.sqrt(sq)) * gs
    norm, coef = _clip(dev, sq, max_norm, gs)
    want_norm, want_coef, bn, bc = OC.clip64(sq, max_norm, gs)
    got_norm, got_coef = float(norm.read("norm")), float(coef.read("coef"))
    assert abs(got_norm - float(want_norm)) <= bn and abs(got_coef - float(want_coef)) <= bc
    assert 0.2 < got_coef < 0.3
    hp = dict(momentum=0.9, dampening=0.0, weight_decay=1e-2, nesterov=False)
    p, buf = _Guarded(dev, n, torch.float32, 7.0, p0), _Guarded(dev, n, torch.float32, float("nan"))
    g = _Guarded(dev, n, torch.float32, 3.0, grads[0])
    assert _sgd(lib, L, p.ptr, g.ptr, buf.ptr, n, LR, hp, True, gs, coef.ptr) == 0
    torch.cuda.synchronize()
    want_p, want_b, bp, bb = OC.sgd_step64(p0, grads[0], None, LR, hp, True, gs, got_coef)   # the device's own coefficient, an fp32 input
    assert OC.within(p.read("p").numpy(), want_p, bp)[0] and OC.within(buf.read("buf").numpy(), want_b, bb)[0]


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_their_code_and_write_nothing(dev, inputs):
    L, lib = _lib()
    n = 1028
    p0, grads = inputs[n]
    p, g = _Guarded(dev, n, torch.float32, 7.0, p0), _Guarded(dev, n, torch.float32, 3.0, grads[0])
    s1, s2 = _Guarded(dev, n, torch.float32, 1.0), _Guarded(dev, n, torch.float32, 2.0)
    sq, part = _Guarded(dev, 1, torch.float64, 5.0), _Guarded(dev, lib.flair_grad_sqnorm_partials(), torch.float64, 5.0)
    nc = _Guarded(dev, 2, torch.float32, 9.0)
    plain = dict(momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False)
    mom = dict(plain, momentum=0.9)
    ahp = OC.adamw_grid()[1]
    st = L.stream()
    calls = [
        (-1, lambda: _sgd(lib, L, None, g.ptr, None, n, LR, plain, True)),
        (-1, lambda: _sgd(lib, L, p.ptr, None, None, n, LR, plain, True)),
        (-1, lambda: _sgd(lib, L, p.ptr, g.ptr, None, n, LR, mom, True)),
        (-1, lambda: _sgd(lib, L, p.ptr, g.ptr, s1.ptr, -1, LR, mom, True)),
        (-2, lambda: _sgd(lib, L, p.ptr, g.ptr, s1.ptr, n, LR, dict(plain, nesterov=True), True)),
        (-2, lambda: _sgd(lib, L, p.ptr, g.ptr, s1.ptr, n, LR, dict(mom, nesterov=True, dampening=0.1), True)),
        (-2, lambda: _sgd(lib, L, p.ptr, g.ptr, s1.ptr, n, LR, dict(mom, momentum=-0.5), True)),
        (-2, lambda: _sgd(lib, L, p.ptr + 4, g.ptr, s1.ptr, n - 4, LR, mom, True)),
        (-1, lambda: _adamw(lib, L, None, g.ptr, s1.ptr, s2.ptr, n, 1e-3, ahp, 1, True)),
        (-1, lambda: _adamw(lib, L, p.ptr, None, s1.ptr, s2.ptr, n, 1e-3, ahp, 1, True)),
        (-1, lambda: _adamw(lib, L, p.ptr, g.ptr, None, s2.ptr, n, 1e-3, ahp, 1, True)),
        (-1, lambda: _adamw(lib, L, p.ptr, g.ptr, s1.ptr, None, n, 1e-3, ahp, 1, True)),
        (-1, lambda: _adamw(lib, L, p.ptr, g.ptr, s1.ptr, s2.ptr, -5, 1e-3, ahp, 1, True)),
        (-2, lambda: _adamw(lib, L, p.ptr, g.ptr, s1.ptr, s2.ptr, n, 1e-3, dict(ahp, betas=(1.0, 0.999)), 1, True)),
        (-2, lambda: _adamw(lib, L, p.ptr, g.ptr, s1.ptr, s2.ptr, n, 1e-3, dict(ahp, betas=(0.9, -0.1)), 1, True)),
        (-2, lambda: _adamw(lib, L, p.ptr, g.ptr, s1.ptr, s2.ptr, n, 1e-3, dict(ahp, betas=(0.9, 1.5)), 1, True)),
        (-1, lambda: lib.flair_grad_sqnorm(None, n, part.ptr, sq.ptr, 0, st)),
        (-1, lambda: lib.flair_grad_sqnorm(g.ptr, n, None, sq.ptr, 0, st)),
        (-1, lambda: lib.flair_grad_sqnorm(g.ptr, n, part.ptr, None, 0, st)),
        (-1, lambda: lib.flair_grad_sqnorm(g.ptr, -1, part.ptr, sq.ptr, 0, st)),
        (-1, lambda: lib.flair_clip_coef(None, 1.0, 1.0, nc.ptr, nc.ptr + 4, st)),
        (-1, lambda: lib.flair_clip_coef(sq.ptr, 1.0, 1.0, None, nc.ptr + 4, st)),
        (-1, lambda: lib.flair_clip_coef(sq.ptr, 1.0, 1.0, nc.ptr, None, st)),
        (-2, lambda: lib.flair_clip_coef(sq.ptr, 1.0, 0.0, nc.ptr, nc.ptr + 4, st)),
    ]
    for i, (want, call) in enumerate(calls):
        assert call() == want, i
    torch.cuda.synchronize()
    for t, name in ((p, "p"), (g, "g"), (s1, "state 1"), (s2, "state 2"), (sq, "sum"), (part, "partials"), (nc, "norm / coef")):
        t.unchanged(name)


def test_ops_wrappers_check_their_arguments(dev):
    from flair_amd import ops
    p, g = torch.zeros(8, device=dev), torch.ones(8, device=dev)
    with pytest.raises(ValueError):
        ops.optim_sgd_(p, torch.ones(4, device=dev), None, 0.1)
    with pytest.raises(ValueError):
        ops.optim_sgd_(p, g, None, 0.1, momentum=0.9)
    with pytest.raises(ValueError):
        ops.optim_sgd_(p, g, torch.zeros(8, device=dev), 0.1, momentum=0.9, dampening=0.1, nesterov=True)
    with pytest.raises(ValueError):
        ops.optim_adamw_(p, g, torch.zeros(8, device=dev), None, 0.1)
    with pytest.raises(ValueError):
        ops.optim_adamw_(p, g, torch.zeros(8, device=dev), torch.zeros(8, device=dev), 0.1, step=0)
    with pytest.raises(ValueError):
        ops.grad_sqnorm_(g, torch.zeros(1, device=dev), torch.zeros(ops.grad_sqnorm_partials(), dtype=torch.float64, device=dev))
    with pytest.raises(ValueError):
        ops.clip_coef_(torch.zeros(1, dtype=torch.float64, device=dev), -1.0, torch.zeros(1, device=dev), torch.zeros(1, device=dev))
    assert torch.equal(p, torch.zeros(8, device=dev))


# ------------------------------------------------------------------------------------------------------------------ the trainer
def _model(dev, seed=2022):
    import flair_amd
    from oracle import unet_resnet34 as om
    hip = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=13, compute_dtype="f32")
    hip.load_state_dict(om.seeded_model(5, 13, seed).state_dict(), strict=True)
    return hip.to(dev).train()


def _batch(seed=0, B=2, S=64):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 5, S, S, generator=g), torch.randint(0, 13, (B, S, S), generator=g, dtype=torch.uint8)


def _seeded_mlp(seed):
    import flair_amd
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        return flair_amd.MetadataMLP()
    finally:
        torch.random.set_rng_state(state)


def _named_norm(trainer, model, extra=None):
    """fp64 norm over the named tensors' gradients (views of trainer.grads at the parameters' offsets), times 1 / world"""
    fo = trainer._opt
    sq = sum(float((trainer.grads[fo.offset(p):fo.offset(p) + p.numel()].double() ** 2).sum()) for p in model.parameters())
    if extra is not None:
        sq += float((extra.double() ** 2).sum())
    return sq


def _check_flat_step(fo, pre_p, pre_state, grads, lr, t, gs, coef):
    """One restated step (fp64 on the device) from the snapshot against what the flat optimizer left"""
    hp = OC.hp_of(fo.spec)
    first = t == 1
    worst = {}
    if fo.spec.name == "sgd":
        want_p, want_b, bp, bb = OC.sgd_step64(pre_p, grads, pre_state[0] if pre_state else None, lr, hp, first, gs, coef)
        pairs = [("p", fo.flat, want_p, bp)] + ([("buf", fo.state[0], want_b, bb)] if pre_state else [])
    else:
        want_p, want_m, want_v, bp, bm, bv = OC.adamw_step64(pre_p, grads, pre_state[0], pre_state[1], lr, hp, t, first, gs, coef)
        pairs = [("p", fo.flat, want_p, bp), ("m", fo.state[0], want_m, bm), ("v", fo.state[1], want_v, bv)]
    for name, got, want, bound in pairs:
        ok, worst[name] = OC.within(got, want, bound)
        assert ok, (t, name, worst[name])
    return worst


def _snapshot(fo):
    return fo.flat.clone(), [s.clone() for s in fo.state]


SPECS = {"sgd-nesterov": (lambda: FO.SGD(momentum=0.9, weight_decay=1e-4, nesterov=True), False),
         "adamw": (lambda: FO.AdamW(), False), "adamw-clip": (lambda: FO.AdamW(), True)}


@pytest.fixture(scope="module")
def first_norm(dev):
    """The gradient norm of the first step of the trainer tests' model and batch, measured once by a plain trainer with lr = 0"""
    import flair_amd
    m = _model(dev)
    tr = flair_amd.SegTrainer(m, lr=0.0)
    x, lab = _batch()
    tr.train_step(x.to(dev), lab.to(dev))
    return float(tr.grads.double().norm())


@pytest.mark.parametrize("which", list(SPECS))
def test_trainer_rules_three_steps(dev, first_norm, which):
    import flair_amd
    make, clip = SPECS[which]
    max_norm = 0.5 * first_norm if clip else None
    m = _model(dev)
    lr = 0.02 if which.startswith("sgd") else 1e-3
    tr = flair_amd.SegTrainer(m, lr=lr, optimizer=make(), clip_grad_norm=max_norm)
    x, lab = _batch()
    x, lab = x.to(dev), lab.to(dev)
    for t in (1, 2, 3):
        pre_p, pre_s = _snapshot(tr._opt)
        tr.train_step(x, lab)
        coef = None
        if clip:
            sq = _named_norm(tr, m)
            want_norm, want_coef, bn, bc = OC.clip64(sq, max_norm)
            # the norm over the flat buffer's runs is the norm over the named tensors (fp64 sums in another order: 2^-24 covers them)
            assert abs(float(tr.grad_norm) - float(want_norm)) <= bn + OC.U * float(want_norm), (float(tr.grad_norm), float(want_norm))
            coef = float(tr._coef)
            assert abs(coef - float(want_coef)) <= bc + 2 * OC.U
            if t == 1:
                assert max_norm < float(tr.grad_norm) and coef < 1.0   # the clip is active
        else:
            assert tr.grad_norm is None
        _check_flat_step(tr._opt, pre_p, pre_s, tr.grads, lr, t, 1.0, coef)
    assert tr._opt.steps == 3


def test_trainer_default_rule_is_the_plain_trainer_bit_for_bit(dev):
    import flair_amd
    a, b = _model(dev), _model(dev)
    ta = flair_amd.SegTrainer(a, lr=0.02, optimizer=FO.SGD())
    tb = flair_amd.SegTrainer(b, lr=0.02)
    assert tb.optimizer is None and tb.grad_norm is None
    x, lab = _batch()
    for _ in range(2):
        la, lb = ta.train_step(x.to(dev), lab.to(dev)).clone(), tb.train_step(x.to(dev), lab.to(dev)).clone()
        assert torch.equal(_bits(la), _bits(lb))
    assert torch.equal(_bits(a.flat_parameters()), _bits(b.flat_parameters()))
    assert torch.equal(_bits(a.flat_buffers()), _bits(b.flat_buffers()))
    assert ta.optimizer_state_dict()["state"] == {}
    with pytest.raises(ValueError):
        tb.optimizer_state_dict()
    with pytest.raises(TypeError):
        flair_amd.SegTrainer(b, lr=0.02, optimizer=torch.optim.SGD(b.parameters(), lr=0.02))


def _plain_step_by_hand(model, tr, img, lab, lr):
    """The plain step call by call, its update by the reference kernel flair_sgd_step (tr lends its head buffers and gradient)"""
    from flair_amd import _lib as L
    from flair_amd import ops
    l = L.lib()
    B, _, H, W = img.shape
    ld = tr._buffers(B, H, W)
    model._c_forward(img, training=True, want_logits=False)
    L.check(l.flair_ce_head_nhwc(l.flair_unet_logits_nhwc(model._h), model._dt, ld, L.ptr(lab), ops._LABEL_KIND[lab.dtype],
                                 L.ptr(tr.class_weight), B, model.classes, H, W, L.ptr(tr.loss), L.ptr(tr._dl), L.ptr(tr._preds), None,
                                 L.ptr(tr.confmat), L.ptr(tr._ce_ws), L.stream()), "ce_head_nhwc")
    model._c_backward(dlogits_nhwc=tr._dl, grads=tr.grads)
    ops.sgd_step_(model._flat_p, tr.grads, lr)
    model._eval.note_native_write()
    return tr.loss.clone()


def _rebind_head_bias(model):
    b = model.segmentation_head[0].bias
    b.data = b.data * 2 + 1          # a new tensor behind the parameter: the next forward rebuilds both flat buffers


def test_plain_trainer_is_the_reference_kernel_and_follows_a_rebuilt_flat_buffer(dev):
    import flair_amd
    lr = 0.02
    a, b = _model(dev), _model(dev)
    ta, lender = flair_amd.SegTrainer(a, lr=lr), flair_amd.SegTrainer(b, lr=lr)
    x, lab = _batch(seed=3, B=1)
    x, lab = x.to(dev), lab.to(dev)
    flats = []
    for step in range(2):
        la = ta.train_step(x, lab).clone()
        lb = _plain_step_by_hand(b, lender, x, lab, lr)
        assert torch.equal(_bits(la), _bits(lb)), (step, float(la), float(lb))
        assert torch.equal(_bits(a.flat_parameters()), _bits(b.flat_parameters())), step
        assert torch.equal(_bits(a.flat_buffers()), _bits(b.flat_buffers())) and torch.equal(a._flat_n, b._flat_n), step
        assert ta._opt.flat is a._flat_p and ta._opt.state == [] and ta._opt.steps == step + 1
        flats.append(a._flat_p)
        _rebind_head_bias(a)
        _rebind_head_bias(b)
    assert flats[0] is not flats[1]                              # the second step did run on a rebuilt buffer
    assert ta.optimizer is None
    # a rule with state cannot follow: its buffers are indexed like the flat parameters they were allocated beside
    c = _model(dev)
    tc = flair_amd.SegTrainer(c, lr=lr, optimizer=FO.SGD(momentum=0.9))
    tc.train_step(x, lab)
    _rebind_head_bias(c)
    with pytest.raises(RuntimeError, match="rebuilt"):
        tc.train_step(x, lab)


def test_trainer_metadata_takes_the_same_rule_and_one_norm(dev):
    import flair_amd
    m, enc = _model(dev), _seeded_mlp(9).to(dev).eval()
    x, lab = _batch(seed=4, B=1, S=512)
    mtd = torch.rand(1, 45, generator=torch.Generator().manual_seed(5))
    x, lab, mtd = x.to(dev), lab.to(dev), mtd.to(dev)
    probe = flair_amd.SegTrainer(m, lr=0.0, metadata_encoder=enc)
    probe.train_step(x, lab, mtd)
    sq0 = float((probe.grads.double() ** 2).sum()) + float((probe.mlp_grads.double() ** 2).sum())
    max_norm = 0.5 * sq0 ** 0.5
    m, enc = _model(dev), _seeded_mlp(9).to(dev).eval()
    lr = 1e-3
    tr = flair_amd.SegTrainer(m, lr=lr, metadata_encoder=enc, optimizer=FO.AdamW(), clip_grad_norm=max_norm)
    start = [p.detach().clone() for p in enc.parameters()]
    for t in (1, 2):
        pre_u, pre_m = _snapshot(tr._opt), _snapshot(tr._mlp_opt)
        tr.train_step(x, lab, mtd)
        assert all(p.grad is None for p in enc.parameters())
        sq = _named_norm(tr, m, tr.mlp_grads)
        want_norm, want_coef, bn, bc = OC.clip64(sq, max_norm)
        assert abs(float(tr.grad_norm) - float(want_norm)) <= bn + OC.U * float(want_norm)
        # the MLP's share is below one fp32 step of the norm here, so it is looked for in the fp64 sum the kernels accumulated:
        # that sum is the named tensors' and the MLP's together to 1e-12, and the MLP's part is a thousand times that
        mlp_sq = float((tr.mlp_grads.double() ** 2).sum())
        assert abs(float(tr._sq) - sq) <= 1e-12 * sq, (float(tr._sq), sq)
        assert mlp_sq > 1e-9 * sq, (mlp_sq, sq)
        coef = float(tr._coef)
        assert abs(coef - float(want_coef)) <= bc + 2 * OC.U
        _check_flat_step(tr._opt, *pre_u, tr.grads, lr, t, 1.0, coef)
        _check_flat_step(tr._mlp_opt, *pre_m, tr.mlp_grads, lr, t, 1.0, coef)
        # the module's parameters ARE the flat copy
        for p in enc.parameters():
            o = tr._mlp_opt.offset(p)
            assert torch.equal(p.detach().reshape(-1), tr._mlp_opt.flat[o:o + p.numel()])
    assert not all(torch.equal(p.detach(), s) for p, s in zip(enc.parameters(), start))
    sd = tr.optimizer_state_dict()
    n_u, n_m = len(list(m.parameters())), len(list(enc.parameters()))
    assert sorted(sd["state"]) == list(range(n_u + n_m))


@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_trainer_state_round_trip(dev, tmp_path, which):
    import flair_amd
    from flair_amd import checkpoint
    make = (lambda: FO.SGD(momentum=0.9, weight_decay=1e-4)) if which == "sgd" else (lambda: FO.AdamW())
    lr = 0.02 if which == "sgd" else 1e-3
    m = _model(dev)
    tr = flair_amd.SegTrainer(m, lr=lr, optimizer=make(), clip_grad_norm=1e6)
    x, lab = _batch()
    x, lab = x.to(dev), lab.to(dev)
    for _ in range(2):
        tr.train_step(x, lab)
    sd = tr.optimizer_state_dict()
    params = list(m.parameters())
    ref = make().torch_optimizer(params, lr)
    assert set(sd["param_groups"][0]) == set(ref.state_dict()["param_groups"][0])
    assert sd["param_groups"][0]["params"] == list(range(len(params)))
    keys = {"momentum_buffer"} if which == "sgd" else {"step", "exp_avg", "exp_avg_sq"}
    for i, p in enumerate(params):
        assert set(sd["state"][i]) == keys
        o = tr._opt.offset(p)
        for key, buf in zip(tr._opt.spec.state_keys, tr._opt.state):
            assert sd["state"][i][key].shape == p.shape
            assert torch.equal(_bits(sd["state"][i][key].reshape(-1)), _bits(buf[o:o + p.numel()]))
        if which == "adamw":
            assert float(sd["state"][i]["step"]) == 2.0
    ref.load_state_dict(sd)   # torch takes it
    assert len(ref.state) == len(params)
    back = make().torch_optimizer(params, lr).state_dict()   # and a dict torch wrote (no state yet) loads here
    fresh_probe = flair_amd.SegTrainer(_model(dev), lr=lr, optimizer=make())
    fresh_probe.load_optimizer_state_dict(back)
    assert fresh_probe._opt.steps == 0
    # through a checkpoint into a fresh trainer: its third step is the original's, bit for bit
    path = str(tmp_path / "state.ckpt")
    checkpoint.save_checkpoint(path, m, optimizer=tr.optimizer, epoch=1, global_step=2)
    m2 = _model(dev, seed=7)
    tr2 = flair_amd.SegTrainer(m2, lr=99.0, optimizer=make(), clip_grad_norm=1e6)
    assert checkpoint.resume(path, m2, optimizer=tr2.optimizer) == (1, 2)
    assert tr2.lr == lr
    m2.train()
    tr.train_step(x, lab)
    tr2.train_step(x, lab)
    assert torch.equal(_bits(m.flat_parameters()), _bits(m2.flat_parameters()))
    for a, b in zip(tr._opt.state, tr2._opt.state):
        assert torch.equal(_bits(a), _bits(b))
    assert tr2._opt.steps == (3 if which == "adamw" else 2)




# ------------------------------------------------------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


DDP_LR = 0.05


def _ddp_spec():
    return FO.SGD(momentum=0.9, weight_decay=1e-2)


def _ddp_worker(rank, port, out_dir):
    """Two steps under a two-rank gloo group on the one GPU.  Each step is checked here against the restatement on the rank's own
    summed gradient with grad_scale = 0.5 (the tensors are too large to hand around); rank 0 also leaves its first step for the
    single-process replay."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    import flair_amd
    dev = torch.device("cuda:0")
    model = _model(dev)
    trainer = flair_amd.SegTrainer(model, lr=DDP_LR, optimizer=_ddp_spec())
    hp = OC.hp_of(trainer._opt.spec)
    x, lab = _batch(seed=30 + rank)
    res = {"steps": []}
    for t in (1, 2):
        pre_p, pre_s = _snapshot(trainer._opt)
        trainer.train_step(x.to(dev), lab.to(dev))
        torch.cuda.synchronize()
        want_p, want_b, bp, bb = OC.sgd_step64(pre_p, trainer.grads, pre_s[0], DDP_LR, hp, t == 1, grad_scale=0.5)
        ok_p, worst_p = OC.within(trainer._opt.flat, want_p, bp)
        ok_b, worst_b = OC.within(trainer._opt.state[0], want_b, bb)
        # what folding 1 / world into lr would have given: the decay term halved as well
        wrong = OC.sgd_step64(pre_p, trainer.grads, pre_s[0], DDP_LR / 2, hp, t == 1)[0]
        res["steps"].append(dict(ok_p=ok_p, worst_p=worst_p, ok_b=ok_b, worst_b=worst_b, fold_ok=OC.within(trainer._opt.flat, wrong, bp)[0],
                                 grads=_bits(trainer.grads).sum().item(), params=_bits(trainer._opt.flat).sum().item()))
        if rank == 0 and t == 1:
            res["first"] = (trainer.grads.cpu(), trainer._opt.flat.cpu(), trainer._opt.state[0].cpu())
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


def test_two_ranks_momentum_and_decay_on_the_averaged_gradient(dev, tmp_path):
    """grad_scale = 1 / world goes on the gradient.  lr / world instead would also halve the decay term: with wd |p| in g' the
    two results differ by lr wd |p| / 2, thousands of times the bound -- this is the test that catches it."""
    import flair_amd
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    res = [torch.load(os.path.join(str(tmp_path), f"rank{r}.pt"), weights_only=False) for r in range(2)]
    for r in range(2):
        for t, s in enumerate(res[r]["steps"], start=1):
            assert s["ok_p"] and s["ok_b"], (r, t, s["worst_p"], s["worst_b"])
            assert not s["fold_ok"], (r, t)
    for a, b in zip(res[0]["steps"], res[1]["steps"]):
        assert a["grads"] == b["grads"] and a["params"] == b["params"]   # the replicas hold the same sum and stay identical
    # single-process replay of the first step: the two batches' gradients from the same start, averaged by grad_scale = 0.5
    start = _model(dev).flat_parameters().detach().clone()
    summed = None
    for r in range(2):
        mm = _model(dev)
        pr = flair_amd.SegTrainer(mm, lr=0.0)
        x, lab = _batch(seed=30 + r)
        pr.train_step(x.to(dev), lab.to(dev))
        summed = pr.grads.clone() if summed is None else summed + pr.grads
    grads0, post_p, post_b = (t.to(dev) for t in res[0]["first"])
    assert torch.equal(_bits(grads0), _bits(summed))   # a + b of the same two fp32 buffers, whoever adds them
    hp = OC.hp_of(_ddp_spec())
    want_p, want_b, bp, bb = OC.sgd_step64(start, summed, None, DDP_LR, hp, True, grad_scale=0.5)
    ok, worst = OC.within(post_p, want_p, bp)
    assert ok, worst
    ok, worst = OC.within(post_b, want_b, bb)
    assert ok, worst
