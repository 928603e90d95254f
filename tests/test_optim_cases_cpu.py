"""The fp64 restatements of tests/optim_cases.py against torch itself, and the host side of flair_amd.optim that needs no device:
specification refusals, the state-dict mapping into and out of torch.optim on CPU tensors, from_config."""
import numpy as np
import pytest
import torch

import optim_cases as OC
from flair_amd import optim as FO

N = 1031
STEPS = 5
LR = 0.05


def _torch_run(make_opt, p0, grads):
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = make_opt([p])
    for g in grads:
        p.grad = torch.from_numpy(g.copy())
        opt.step()
    return p.detach().numpy(), opt


@pytest.mark.parametrize("hp", OC.sgd_grid(), ids=lambda hp: OC.case_id(("sgd", hp, False)))
def test_sgd_restatement_against_torch(hp):
    p0 = OC.rand_f32(N, 1)
    grads = [OC.rand_f32(N, 10 + s) for s in range(STEPS)]
    got, opt = _torch_run(lambda ps: torch.optim.SGD(ps, lr=LR, **hp), p0, grads)
    p, buf = p0.astype(np.float64), None
    sum_p, sum_b = 0.0, 0.0
    for s, g in enumerate(grads):
        p, buf, bound_p, bound_b = OC.sgd_step64(p, g, buf, LR, hp, first=s == 0, round_hyper=False)
        sum_p, sum_b = sum_p + bound_p, sum_b + bound_b + OC.U * np.abs(g)
    # torch rounds every operation of every step to fp32 where the restatement never does: the one-step bound once per step, each
    # at that step's magnitudes (a parameter that ends near zero still carries the roundings of the steps it was large in); an
    # error in the buffer reaches the parameter through lr (1 + momentum)
    assert np.all(np.abs(got - p) <= sum_p + STEPS * LR * 2 * sum_b), float(np.max(np.abs(got - p) / sum_p))
    if hp["momentum"] != 0:
        tb = opt.state_dict()["state"][0]["momentum_buffer"].numpy()
        assert np.all(np.abs(tb - buf) <= sum_b + hp["weight_decay"] * sum_p), float(np.max(np.abs(tb - buf) / sum_b))


@pytest.mark.parametrize("hp", OC.adamw_grid(), ids=lambda hp: OC.case_id(("adamw", hp, False)))
def test_adamw_restatement_against_torch(hp):
    p0 = OC.rand_f32(N, 2)
    grads = [OC.rand_f32(N, 20 + s, scale=0.1) for s in range(STEPS)]
    lr = 1e-3
    got, opt = _torch_run(lambda ps: torch.optim.AdamW(ps, lr=lr, **hp), p0, grads)
    p, m, v = p0.astype(np.float64), None, None
    sum_p, sum_m, sum_v = 0.0, 0.0, 0.0
    for s, g in enumerate(grads):
        p, m, v, bound_p, bound_m, bound_v = OC.adamw_step64(p, g, m, v, lr, hp, t=s + 1, first=s == 0, round_hyper=False)
        sum_p, sum_m, sum_v = sum_p + bound_p + OC.U * np.abs(p), sum_m + bound_m, sum_v + bound_v
    st = opt.state_dict()["state"][0]
    # the one-step bounds once per step, each at that step's magnitudes; torch rounds p (1 - lr wd) and the subtraction of the
    # step separately, one rounding on |p| more than the kernel's fma, which the bound counts
    assert np.all(np.abs(got - p) <= sum_p), float(np.max(np.abs(got - p) / sum_p))
    assert np.all(np.abs(st["exp_avg"].numpy() - m) <= sum_m), float(np.max(np.abs(st["exp_avg"].numpy() - m) / sum_m))
    assert np.all(np.abs(st["exp_avg_sq"].numpy() - v) <= sum_v), float(np.max(np.abs(st["exp_avg_sq"].numpy() - v) / sum_v))
    assert float(st["step"]) == STEPS


@pytest.mark.parametrize("max_norm", [0.5, 1e4])
def test_clip_restatement_against_torch(max_norm):
    gs = [OC.rand_f32(257, 3), OC.rand_f32(1031, 4)]
    ps = [torch.nn.Parameter(torch.zeros(g.size)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = torch.from_numpy(g.copy())
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    norm, coef, bn, bc = OC.clip64(OC.sqnorm64(*gs), max_norm)
    assert abs(float(total) - float(norm)) <= bn + 2 * OC.U * float(norm)   # torch's own norm is an fp32 reduction
    assert (coef == 1.0) == (max_norm > float(norm))
    for p, g in zip(ps, gs):
        want = g.astype(np.float64) * float(coef)
        assert np.all(np.abs(p.grad.numpy() - want) <= (4 + 1) * OC.U * np.abs(want) + bc * np.abs(g))


def test_specification_refusals():
    for kw, msg in ((dict(momentum=-0.1), "Invalid momentum value"), (dict(weight_decay=-1.0), "Invalid weight_decay value"),
                    (dict(nesterov=True), "Nesterov momentum requires"), (dict(nesterov=True, momentum=0.9, dampening=0.1), "Nesterov")):
        with pytest.raises(ValueError, match=msg):
            FO.SGD(**kw)
        with pytest.raises(ValueError, match=msg):   # torch's own rule and message
            torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1, **kw)
    for kw, msg in ((dict(betas=(1.0, 0.999)), "Invalid beta parameter at index 0"), (dict(betas=(0.9, -0.1)), "Invalid beta parameter at index 1"),
                    (dict(eps=-1e-8), "Invalid epsilon value"), (dict(weight_decay=-0.1), "Invalid weight_decay value")):
        with pytest.raises(ValueError, match=msg):
            FO.AdamW(**kw)
        with pytest.raises(ValueError, match=msg):
            torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=0.1, **kw)
    with pytest.raises(ValueError):
        FO.AdamW(betas=(0.9,))
    with pytest.raises(ValueError):
        FO.FlatOptimizer(FO.SGD(), torch.zeros(8, dtype=torch.float64), [])
    with pytest.raises(ValueError):   # a parameter that is no view of the flat buffer
        FO.FlatOptimizer(FO.SGD(momentum=0.9), torch.zeros(8), [torch.nn.Parameter(torch.zeros(4))])


def _bound(spec, shapes):
    """A FlatOptimizer on CPU tensors: parameters as views of one flat buffer, 4-float padding between them"""
    offs, n = [], 0
    for s in shapes:
        offs.append(n)
        n += -(-int(np.prod(s)) // 4) * 4
    flat = torch.from_numpy(OC.rand_f32(n, 5))
    params = []
    for s, o in zip(shapes, offs):
        p = torch.nn.Parameter(torch.zeros(s))
        p.data = flat[o:o + int(np.prod(s))].view(s)
        params.append(p)
    return FO.FlatOptimizer(spec, flat, params), params


SHAPES = [(3, 5), (7,), (2, 2, 4)]


@pytest.mark.parametrize("spec", [FO.SGD(momentum=0.9, weight_decay=1e-4, nesterov=True), FO.AdamW()], ids=["sgd", "adamw"])
def test_state_dict_into_torch_optim(spec):
    fo, params = _bound(spec, SHAPES)
    extra = torch.nn.Parameter(torch.zeros(3))   # a parameter no flat optimizer holds: listed, without state
    for k, buf in enumerate(fo.state):
        buf.copy_(torch.from_numpy(np.abs(OC.rand_f32(buf.numel(), 30 + k))))
    fo.steps = 2
    top = FO.TrainerOptimizer(spec, lambda: [fo], params + [extra], lambda: 0.03)
    sd = top.state_dict()
    ref = spec.torch_optimizer(params + [extra], 0.03)
    assert set(sd["param_groups"][0]) == set(ref.state_dict()["param_groups"][0])
    assert sd["param_groups"][0]["params"] == [0, 1, 2, 3] and sd["param_groups"][0]["lr"] == 0.03
    assert sorted(sd["state"]) == [0, 1, 2]
    ref.load_state_dict(sd)
    for p in params:
        st = ref.state[p]
        o = fo.offset(p)
        for key, buf in zip(spec.state_keys, fo.state):
            assert st[key].shape == p.shape
            assert torch.equal(st[key].reshape(-1), buf[o:o + p.numel()])
            assert st[key].data_ptr() != buf[o:].data_ptr()   # clones, not views
        if spec.name == "adamw":
            assert float(st["step"]) == 2.0


@pytest.mark.parametrize("spec", [FO.SGD(momentum=0.9), FO.AdamW(weight_decay=0.0)], ids=["sgd", "adamw"])
def test_state_dict_out_of_torch_optim(spec):
    fo, params = _bound(spec, SHAPES)
    ref = spec.torch_optimizer(params, 0.01)
    for s in range(3):
        for k, p in enumerate(params):
            p.grad = torch.from_numpy(OC.rand_f32(p.numel(), 40 + 3 * s + k)).view(p.shape)
        ref.step()
    lrs = []
    top = FO.TrainerOptimizer(spec, lambda: [fo], params, lambda: 0.5, lrs.append)
    top.load_state_dict(ref.state_dict())
    assert lrs == [0.01]   # torch restores the learning rate with the state
    assert fo.steps == (3 if spec.name == "adamw" else 1)   # momentum SGD keeps no count: "not the first step" is all it needs
    for p in params:
        o = fo.offset(p)
        for key, buf in zip(spec.state_keys, fo.state):
            assert torch.equal(ref.state[p][key].reshape(-1), buf[o:o + p.numel()])
    back = top.state_dict()
    for i, p in enumerate(params):
        for key in spec.state_keys:
            assert torch.equal(back["state"][i][key], ref.state[p][key])
    with pytest.raises(ValueError):   # written by another rule
        other = FO.SGD(momentum=0.5) if spec.name == "sgd" else FO.AdamW(betas=(0.8, 0.999), weight_decay=0.0)
        FO.TrainerOptimizer(other, lambda: [fo], params, lambda: 0.5).load_state_dict(ref.state_dict())


def test_state_dict_before_the_first_step_is_empty():
    fo, params = _bound(FO.AdamW(), SHAPES)
    sd = FO.TrainerOptimizer(fo.spec, lambda: [fo], params, lambda: 0.1).state_dict()
    assert sd["state"] == {}
    fo.spec.torch_optimizer(params, 0.1).load_state_dict(sd)
    fo2, params2 = _bound(FO.SGD(), SHAPES)   # plain SGD has no state at any step
    fo2.steps = 4
    assert FO.TrainerOptimizer(fo2.spec, lambda: [fo2], params2, lambda: 0.1).state_dict()["state"] == {}


def test_from_config():
    s = FO.from_config({"learning_rate": 0.02})
    assert isinstance(s, FO.SGD) and (s.momentum, s.dampening, s.weight_decay, s.nesterov) == (0.0, 0.0, 0.0, False)
    s = FO.from_config({"optimizer": {"name": "sgd", "momentum": 0.9, "nesterov": True, "weight_decay": 1e-4}})
    assert isinstance(s, FO.SGD) and (s.momentum, s.nesterov, s.weight_decay) == (0.9, True, 1e-4)
    s = FO.from_config({"optimizer": {"name": "AdamW", "betas": [0.8, 0.99], "eps": 1e-6}})
    assert isinstance(s, FO.AdamW) and (s.betas, s.eps, s.weight_decay) == ((0.8, 0.99), 1e-6, 1e-2)
    for bad in ({"name": "lion"}, {"momentum": 0.9}, {"name": "sgd", "lr": 0.1}, "sgd"):
        with pytest.raises(ValueError):
            FO.from_config({"optimizer": bad})
    ps = [torch.nn.Parameter(torch.zeros(2))]
    o = FO.torch_optimizer_from_config({"learning_rate": 0.02}, ps)
    assert type(o) is torch.optim.SGD
    assert o.state_dict()["param_groups"] == torch.optim.SGD(ps, lr=0.02).state_dict()["param_groups"]
    o = FO.torch_optimizer_from_config({"learning_rate": 0.02, "optimizer": {"name": "adamw", "weight_decay": 0.05}}, ps)
    assert type(o) is torch.optim.AdamW and o.param_groups[0]["weight_decay"] == 0.05 and o.param_groups[0]["lr"] == 0.02


def test_get_segmentation_module_reads_the_optimizer_key():
    from flair_amd.tasks_utils import get_segmentation_module
    cfg = {"model_framework": {"model_provider": "SegmentationModelsPytorch",
                               "SegmentationModelsPytorch": {"encoder_decoder": "resnet34_unet", "encoder_weights": None}},
           "use_metadata": False, "use_weights": False, "channels": [1, 2, 3, 4, 5],
           "classes": {i + 1: [1, f"class{i + 1}"] for i in range(13)}, "learning_rate": 0.02}
    plain = get_segmentation_module(cfg, "train").optimizer
    assert type(plain) is torch.optim.SGD   # without the key: torch.optim.SGD(lr), as before
    want = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.02).state_dict()["param_groups"][0]
    got = plain.state_dict()["param_groups"][0]
    assert {k: v for k, v in got.items() if k != "params"} == {k: v for k, v in want.items() if k != "params"}
    task = get_segmentation_module(dict(cfg, optimizer={"name": "adamw", "betas": [0.8, 0.99], "weight_decay": 0.05}), "train")
    g = task.optimizer.param_groups[0]
    assert type(task.optimizer) is torch.optim.AdamW and (tuple(g["betas"]), g["weight_decay"], g["lr"]) == ((0.8, 0.99), 0.05, 0.02)
    assert len(g["params"]) == len(list(task.model.parameters()))
    task = get_segmentation_module(dict(cfg, optimizer={"name": "sgd", "momentum": 0.9, "nesterov": True}), "train")
    g = task.optimizer.param_groups[0]
    assert type(task.optimizer) is torch.optim.SGD and (g["momentum"], g["nesterov"], g["lr"]) == (0.9, True, 0.02)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_update_scales_keeps_both_ways_of_averaging_over_the_ranks(world):
    """The plain trainer's p -= f32(lr / world) * sum g and the other rules' p -= f32(lr) * (sum g * f32(1 / world)) differ in the last
    bit when world is no power of two: each keeps its own pair, as Python floats, and a scale of exactly 1.0 selects the unscaled kernel."""
    from flair_amd.train import update_scales
    lr = 0.05
    assert update_scales(lr, world, True) == (lr / world, 1.0)
    assert update_scales(lr, world, False) == (lr, 1.0 / world)
    assert all(type(v) is float for fold in (True, False) for v in update_scales(lr, world, fold))
