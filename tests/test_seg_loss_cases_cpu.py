"""No GPU: the specification of the configurable loss (flair_amd/losses.py), its place in the host layers, and the cases of the
operator tests (tests/seg_loss_cases.py, run by test_gpu_seg_loss.py).  The fp64 reference is held against torch's own label-smoothed
cross entropy and against the cross-entropy head's reference; the closed-form Dice gradient the kernels use against autograd; the
kernels' arithmetic, restated in fp32, stays inside the GPU test's bounds with 4x to spare on every case, and fp32 and fp64 argmax
agree on every pixel."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ce_head_cases as K
import seg_loss_cases as S

SPARE = 4.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the specification
def test_specification_defaults_repr_and_tuple():
    from flair_amd import SegLoss, losses
    s = SegLoss()
    assert s.astuple() == (1.0, 0.0, 0.0, 0.0, 0.0, 1e-7)
    assert repr(s) == "SegLoss(ce=1.0, label_smoothing=0.0, focal_gamma=0.0, dice=0.0, dice_smooth=0.0, dice_eps=1e-07)"
    assert SegLoss(dice=0.5, dice_smooth=1) == SegLoss(dice=0.5, dice_smooth=1.0) and SegLoss() != SegLoss(dice=1)
    assert losses.SegLoss is SegLoss
    for name, kw in S.SPECS.items():
        assert isinstance(S.spec_of(name), SegLoss), name
        assert eval(repr(S.spec_of(name)), {"SegLoss": SegLoss}) == S.spec_of(name)


@pytest.mark.parametrize("kw,named", [
    (dict(ce=-1), "ce"), (dict(dice=-0.5), "dice"), (dict(ce=0, dice=0), "ce"), (dict(ce=0, dice=0), "dice"),
    (dict(label_smoothing=-0.1), "label_smoothing"), (dict(label_smoothing=1.0), "label_smoothing"),
    (dict(focal_gamma=0.5), "focal_gamma"), (dict(focal_gamma=-1), "focal_gamma"),
    (dict(label_smoothing=0.1, focal_gamma=2), "label_smoothing"), (dict(label_smoothing=0.1, focal_gamma=2), "focal_gamma"),
    (dict(ce=0, dice=1, label_smoothing=0.1), "label_smoothing"), (dict(ce=0, dice=1, focal_gamma=2), "focal_gamma"),
    (dict(dice=1, dice_smooth=-1), "dice_smooth"), (dict(dice=1, dice_eps=0), "dice_eps"), (dict(dice=1, dice_eps=-1e-7), "dice_eps"),
    (dict(ce=float("nan")), "ce"), (dict(dice=float("inf")), "dice"),
])
def test_specification_refuses_and_names_the_argument(kw, named):
    from flair_amd import SegLoss
    with pytest.raises(ValueError, match=named):
        SegLoss(**kw)


def test_specification_accepts_the_edges():
    from flair_amd import SegLoss
    SegLoss(focal_gamma=1.0)
    SegLoss(label_smoothing=0.999)
    SegLoss(ce=0, dice=2.0)
    SegLoss(dice=1, dice_smooth=0.0, dice_eps=1e-12)


def test_from_config():
    from flair_amd import SegLoss, losses
    assert losses.from_config({}) is None and losses.from_config({"loss": None}) is None
    assert losses.from_config({"loss": {}}) == SegLoss()
    got = losses.from_config({"loss": {"ce": 1, "dice": 0.5, "label_smoothing": 0.1, "dice_smooth": 1, "dice_eps": 1e-6}})
    assert got == SegLoss(ce=1.0, dice=0.5, label_smoothing=0.1, dice_smooth=1.0, dice_eps=1e-6)
    assert losses.from_config({"loss": {"focal_gamma": 2}}) == SegLoss(focal_gamma=2.0)
    with pytest.raises(ValueError, match="gamma"):
        losses.from_config({"loss": {"gamma": 2}})
    with pytest.raises(ValueError, match="mapping"):
        losses.from_config({"loss": "dice"})
    with pytest.raises(ValueError, match="focal_gamma"):
        losses.from_config({"loss": {"focal_gamma": 0.3}})


def test_entry_points_are_declared_and_bound():
    from flair_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "flair_hip.h")).read()
    for name in ("flair_seg_loss_workspace_bytes", "flair_seg_loss", "flair_seg_loss_nhwc"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in L.PROTOTYPES
    assert "flair_seg_loss_t" in header
    # the declared parameter counts are the bound ones
    for name in ("flair_seg_loss_workspace_bytes", "flair_seg_loss", "flair_seg_loss_nhwc"):
        decl = re.search(r"\b%s\(([^;]*)\);" % name, header).group(1)
        assert len(decl.split(",")) == len(L.PROTOTYPES[name][1]), name
    assert [f[0] for f in L.SegLossSpec._fields_] == ["ce", "label_smoothing", "focal_gamma", "dice", "dice_smooth", "dice_eps"]
    import ctypes
    assert ctypes.sizeof(L.SegLossSpec) == 24
    capi = open(os.path.join(ROOT, "flair-1_amd", "csrc", "capi.hip")).read()
    assert "case -20:" in capi and "flair_seg_loss_t" in capi
    build_py = open(os.path.join(ROOT, "flair-1_amd", "build.py")).read()
    assert '"seg_loss.hip"' in build_py


def _config(**extra):
    cfg = {"model_framework": {"model_provider": "SegmentationModelsPytorch",
                               "SegmentationModelsPytorch": {"encoder_decoder": "resnet34_unet"}},
           "channels": [1, 2, 3, 4, 5], "norm_type": "custom", "use_metadata": False, "use_weights": True, "learning_rate": 0.02,
           "classes": {i + 1: [1.0 if i < 12 else 0.0, f"class{i}"] for i in range(13)}}
    cfg.update(extra)
    return cfg


def _criterion(cfg, monkeypatch):
    """The criterion get_segmentation_module builds, with the model factory replaced by a one-layer stand-in (no device needed)."""
    from flair_amd import tasks_utils
    monkeypatch.setattr(tasks_utils, "FLAIR_ModelFactory", lambda config, **kw: torch.nn.Conv2d(5, 13, 1))
    return tasks_utils.get_segmentation_module(cfg, stage="train").criterion


def test_get_segmentation_module_without_loss_builds_todays_criterion(monkeypatch):
    from flair_amd import FusedCrossEntropyLoss
    crit = _criterion(_config(), monkeypatch)
    assert type(crit) is FusedCrossEntropyLoss and not hasattr(crit, "spec")
    assert torch.equal(crit.weight, torch.tensor([1.0] * 12 + [0.0]))
    assert type(_criterion(_config(use_weights=False), monkeypatch)) is FusedCrossEntropyLoss


def test_get_segmentation_module_with_loss_builds_the_fused_seg_loss(monkeypatch):
    from flair_amd import FusedSegLoss, SegLoss
    crit = _criterion(_config(loss={"dice": 1.0, "label_smoothing": 0.1}), monkeypatch)
    assert type(crit) is FusedSegLoss and crit.spec == SegLoss(dice=1.0, label_smoothing=0.1)
    assert torch.equal(crit.weight, torch.tensor([1.0] * 12 + [0.0]))
    assert _criterion(_config(use_weights=False, loss={"focal_gamma": 2}), monkeypatch).weight is None
    with pytest.raises(TypeError):
        FusedSegLoss({"dice": 1.0})


# ------------------------------------------------------------------------------------------------ the reference against torch
@pytest.mark.parametrize("C,shape,family,weight", [(13, S.SMALL, "ints", "none"), (19, S.MEDIUM, "far", "rand"),
                                                   (19, S.MEDIUM, "ints", "zeros"), (2, S.SMALL, "far", "rand")])
def test_reference_with_smoothing_is_torchs_cross_entropy(C, shape, family, weight):
    from flair_amd import SegLoss
    v = K.case_values(C, shape, family, weight)
    for kind in ("i64", "onehot"):
        y, valid = S.labels_and_valid(v["lab"], kind)
        for eps in (0.1, 0.35):
            ref = S.reference_of(v["x"], y, valid, v["w"], SegLoss(label_smoothing=eps))
            xd = v["x"].double().requires_grad_(True)
            tgt = torch.where(valid, y, torch.full_like(y, -100))
            want = F.cross_entropy(xd, tgt, weight=None if v["w"] is None else v["w"].double(), ignore_index=-100, label_smoothing=eps)
            (dl,) = torch.autograd.grad(want, xd)
            want = float(want.detach())
            assert abs(ref["loss"] - want) <= 1e-12 * max(1.0, abs(want)), (kind, eps, ref["loss"], want)
            assert float((ref["dl"] - dl).abs().max()) <= 1e-12
            assert ref["ce"] == ref["loss"] and ref["dice"] == 0.0


@pytest.mark.parametrize("C,shape,family,weight", [(13, S.SMALL, "ints", "rand"), (19, S.MEDIUM, "far", "zeros"), (32, S.SMALL, "far", "none")])
def test_reference_of_the_default_specification_is_the_ce_heads(C, shape, family, weight):
    from flair_amd import SegLoss
    v = K.case_values(C, shape, family, weight)
    for kind, which in (("i32", "int"), ("onehot", "onehot")):
        y, valid = S.labels_and_valid(v["lab"], kind)
        ref = S.reference_of(v["x"], y, valid, v["w"], SegLoss())
        assert abs(ref["loss"] - v[which]["loss"]) <= 1e-12 * max(1.0, abs(ref["loss"]))
        assert float((ref["dl"] - v[which]["dl"]).abs().max()) <= 1e-14
        assert ref["ce"] == ref["loss"]


@pytest.mark.parametrize("C,shape,family,weight,kind,smooth", [(13, S.MEDIUM, "ints", "rand", "i64", 0.0), (19, S.SMALL, "far", "zeros", "onehot", 1.0),
                                                               (2, S.SMALL, "ints", "none", "u8", 0.0), (32, S.MEDIUM, "far", "none", "i32", 1.0)])
def test_closed_form_dice_gradient_is_autograds(C, shape, family, weight, kind, smooth):
    from flair_amd import SegLoss
    v = K.case_values(C, shape, family, weight)
    y, valid = S.labels_and_valid(v["lab"], kind)
    spec = SegLoss(ce=0.0, dice=0.7, dice_smooth=smooth)
    ref = S.reference_of(v["x"], y, valid, v["w"], spec)
    got = S.dice_gradient_closed_form(v["x"], y, valid, v["w"], spec)
    assert float(ref["dl"].abs().max()) > 0
    assert float((got - ref["dl"]).abs().max()) <= 1e-14 * max(1.0, float(ref["dl"].abs().max()) * 1e3)


def test_dice_reference_edges():
    """No counted pixel: the term and its gradient are 0.  One-hot softmax on the labels: the term is 0."""
    from flair_amd import SegLoss
    spec = SegLoss(ce=0.0, dice=1.0)
    win = S.exact_winners()
    x = S.exact_logits(win, S.EXACT_C)
    none = S.reference_of(x, win, torch.zeros_like(win, dtype=torch.bool), None, spec)
    assert none["loss"] == 0.0 and float(none["dl"].abs().max()) == 0.0
    hit = S.reference_of(x, win, torch.ones_like(win, dtype=torch.bool), None, spec)
    assert abs(hit["loss"]) <= 1e-15 and float(hit["dl"].abs().max()) <= 1e-15
    r32 = S.kernel_arithmetic_f32(x, win, torch.ones_like(win, dtype=torch.bool), None, spec)
    assert r32["loss"] == 0.0 and float(r32["dl"].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ the restatement and the table
@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_fp32_arithmetic_stays_inside_the_bounds_with_room(case):
    v, y, valid, ref = S.case_reference(case)
    spec = S.spec_of(case.spec)
    r = S.kernel_arithmetic_f32(v["x"], y, valid, v["w"], spec)
    for key in ("loss", "ce", "dice"):
        err, bound = abs(r[key] - ref[key]), S.loss_bound(ref[key])
        print(f"{case.name} {key}: fp64 {ref[key]:.9f} err {err:.2e} (bound {bound:.2e})")
        assert np.isfinite(ref[key]) and err * SPARE <= bound, (key, err, bound)
    de, db, mx = float((r["dl"].double() - ref["dl"]).abs().max()), S.dl_bound(ref["dl"]), float(ref["dl"].abs().max())
    print(f"{case.name}: dl err {de:.2e} (bound {db:.2e}), relative to max |dl| {de / mx:.2e}")
    assert mx > 0 and bool(torch.isfinite(ref["dl"]).all())
    assert de * SPARE <= db, (de, db)
    ce_ref = v["onehot" if case.kind == "onehot" else "int"]
    assert torch.equal(r["preds"], ce_ref["preds"]), "fp32 and fp64 argmax differ"
    # an ignored pixel carries no gradient; with Dice alone neither does a pixel of a class that weighs nothing
    if (~valid).any():
        assert float(ref["dl"].permute(0, 2, 3, 1)[~valid].abs().max()) == 0.0
    assert (ref["ce"] != 0) == (spec.ce > 0) and (ref["dice"] != 0) == (spec.dice > 0)


def test_the_table_covers_what_the_issue_names():
    cs = S.CASES
    assert {c.C for c in cs} == {2, 13, 19, 32}
    assert {c.shape for c in cs} == {S.SMALL, S.MEDIUM, S.LARGE} and S.LARGE == (3, 419, 421)
    assert {c.family for c in cs} == {"ints", "far"} and {c.weight for c in cs} == {"none", "rand", "zeros"}
    assert {c.kind for c in cs} == set(K.KINDS) and {c.spec for c in cs} == set(S.SPECS)
    assert all(c.C == 19 for c in cs if c.weight == "zeros")
    assert all(c.ld in (16, 32) and c.ld >= c.C for c in cs)
    assert {(c.C, c.ld) for c in cs} >= {(13, 16), (13, 32), (2, 16), (2, 32), (19, 32), (32, 32)}
    assert len({c.name for c in cs}) == len(cs)
    # pairwise: every specification meets both families, two class counts and two label kinds; every class count every shape class
    for name in S.SPECS:
        mine = [c for c in cs if c.spec == name]
        assert {c.family for c in mine} == {"ints", "far"} and len({c.C for c in mine}) >= 2 and len({c.kind for c in mine}) >= 2, name
    for C in (2, 13, 19, 32):
        assert {c.shape for c in cs if c.C == C} >= {S.SMALL, S.MEDIUM} or C == 19, C
    large = [c for c in cs if c.shape == S.LARGE]
    assert len(large) == 2 and {c.ld for c in large} == {16, 32} and any(S.SPECS[c.spec].get("dice") for c in large)
    B, H, W = S.LARGE
    assert B * H * W > K.CE_BLOCK_CAP * 256 and (H * W) % 4
    specs = {n: S.spec_of(n) for n in S.SPECS}
    assert specs["ls"].label_smoothing == pytest.approx(0.1) and specs["focal2"].focal_gamma == 2 and specs["focal15"].focal_gamma == 1.5
    assert specs["dice"].ce == 0 and specs["dice"].dice_smooth == 0 and specs["dice_s1"].dice_smooth == 1
    assert specs["ce_dice_ls"].ce > 0 and specs["ce_dice_ls"].dice > 0 and specs["ce_dice_ls"].label_smoothing > 0
