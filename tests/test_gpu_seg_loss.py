"""The head with a configurable objective (csrc/seg_loss.hip: flair_seg_loss, flair_seg_loss_nhwc) against the fp64 reference of
tests/seg_loss_cases.py, and the layers above it: ops.seg_loss, head.FusedSegLoss, task_module.fused_step, SegTrainer(loss=...).

Operator runs keep every output inside a guarded allocation (the helpers of test_gpu_ce_head_exact.py) and a workspace of exactly
flair_seg_loss_workspace_bytes.  Predictions and confusion matrices are compared with flair_ce_head(_nhwc)'s on the same tensors
for equality; loss, terms and gradient with the reference inside the bounds test_seg_loss_cases_cpu.py justifies; bf16 rows are
bit for bit the round-to-nearest-even of the fp32 rows, as the cross-entropy head's are."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ce_head_cases as K
import seg_loss_cases as S
import test_gpu_ce_head_exact as CE      # its guarded buffers and its flair_ce_head(_nhwc) runs

pytestmark = pytest.mark.gpu

_bits, _Guarded = CE._bits, CE._Guarded
TDT, KIND_CODE, JUNK, CM_FILL, GUARD_ROWS = CE.TDT, CE.KIND_CODE, CE.JUNK, CE.CM_FILL, CE.GUARD_ROWS
LAYOUTS = ("nchw", "f32", "bf16")


def _spec_c(spec):
    from flair_amd import ops
    return ops.seg_loss_spec(spec)


def run_seg(dev, C, shape, x, labels, kind, w, spec, layout, ld=0, want_dl=True):
    """flair_seg_loss (layout "nchw") or flair_seg_loss_nhwc (fp32 / bf16 rows of stride ld) on guarded buffers -> dict terms (3,),
    preds (npix,), cm (C, C) counted, dl (npix, C | ld) or None."""
    L = CE._lib()
    l = L.lib()
    B, H, W = shape
    npix = B * H * W
    o = {"terms": _Guarded(dev, 3, torch.float32, 7.0, guard=4), "preds": _Guarded(dev, npix, torch.uint8, 0xA5),
         "targets": _Guarded(dev, npix, torch.int32, 0x5A5A5A5A), "cm": _Guarded(dev, C * C, torch.int64, -7, guard=8)}
    CE._fill_cm(o)
    nws = l.flair_seg_loss_workspace_bytes(B, C, H, W)
    assert nws % 4 == 0 and nws > l.flair_ce_workspace_bytes(B, H, W)
    ws = _Guarded(dev, nws, torch.uint8, 0xC3)
    wd = None if w is None else w.to(dev)
    sp = _spec_c(spec)
    if layout == "nchw":
        xin = x.to(dev).contiguous()
        dl = _Guarded(dev, x.numel(), torch.float32, float("nan"))
        rc = l.flair_seg_loss(L.ptr(xin), L.ptr(labels), KIND_CODE[kind], L.ptr(wd), B, C, H, W, ctypes.byref(sp), o["terms"].ptr,
                              dl.ptr if want_dl else None, o["preds"].ptr, None, o["targets"].ptr, o["cm"].ptr, ws.ptr, L.stream())
    else:
        dt = TDT[layout]
        rows = K.nhwc_rows(x, ld, fill=JUNK).to(device=dev, dtype=dt)
        dl = _Guarded(dev, npix * ld, dt, float("nan"), guard=GUARD_ROWS * ld)
        assert rows.data_ptr() % 16 == 0 and dl.ptr % 16 == 0
        rc = l.flair_seg_loss_nhwc(rows.data_ptr(), L.dtype_code(dt), ld, L.ptr(labels), KIND_CODE[kind], L.ptr(wd), B, C, H, W,
                                   ctypes.byref(sp), o["terms"].ptr, dl.ptr if want_dl else None, o["preds"].ptr, o["targets"].ptr,
                                   o["cm"].ptr, ws.ptr, L.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    what = f"seg_loss {layout} ld{ld}"
    ws.read(what + " workspace")
    r = {"terms": o["terms"].read(what + " terms"), "preds": o["preds"].read(what + " preds"),
         "targets": o["targets"].read(what + " targets"), "cm": o["cm"].read(what + " confmat").view(C, C) - CM_FILL}
    d = dl.read(what + " dlogits")
    if layout == "nchw":
        r["dl"] = d.view(B, C, H, W).permute(0, 2, 3, 1).reshape(-1, C)
    else:
        r["dl"] = d.view(npix, ld)
    return r


def check_terms(r, ref, what):
    for i, key in enumerate(("loss", "ce", "dice")):
        got, err, bound = float(r["terms"][i]), abs(float(r["terms"][i]) - ref[key]), S.loss_bound(ref[key])
        print(f"{what} {key}: {got:.9f} fp64 {ref[key]:.9f} err {err:.2e} (bound {bound:.2e})")
        assert np.isfinite(got) and err <= bound, (what, key, got, ref[key])


def check_dl(dl, ref_dl, C, valid, what):
    rows = ref_dl.permute(0, 2, 3, 1).reshape(-1, C)
    err, bound = float((dl[:, :C].double() - rows).abs().max()), S.dl_bound(ref_dl)
    print(f"{what}: max |dl - fp64| {err:.2e} (bound {bound:.2e})")
    assert err <= bound, (what, err, bound)
    CE.check_rows(dl, C, valid, what)


# ------------------------------------------------------------------------------------------------ operator parity
@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_operator_against_the_fp64_reference_and_the_ce_head(dev, case):
    v, y, valid, ref = S.case_reference(case)
    C, ld, shape, kind = case.C, case.ld, case.shape, case.kind
    spec = S.spec_of(case.spec)
    labels = v["lab"][kind].to(dev).contiguous()
    got = {lay: run_seg(dev, C, shape, v["x"], labels, kind, v["w"], spec, lay, ld) for lay in LAYOUTS}
    ce = {"nchw": CE.run_nchw(dev, C, shape, v["x"], labels, kind, v["w"], want_dl=False)}
    for dt in ("f32", "bf16"):
        ce[dt] = CE.run_nhwc(dev, C, ld, shape, v["x"], labels, kind, v["w"], dt, want_dl=False)
    for lay in LAYOUTS:
        what = f"{case.name} {lay}"
        check_terms(got[lay], ref, what)
        assert torch.equal(got[lay]["preds"], ce[lay]["preds"]), f"{what}: preds differ from the CE head's"
        assert torch.equal(got[lay]["cm"], ce[lay]["cm"]), f"{what}: confusion matrix differs from the CE head's"
        assert torch.equal(got[lay]["targets"], ce[lay]["targets"]), f"{what}: targets"
    check_dl(got["nchw"]["dl"], ref["dl"], C, valid, f"{case.name} nchw")
    check_dl(got["f32"]["dl"], ref["dl"], C, valid, f"{case.name} f32")
    CE.check_rows(got["bf16"]["dl"], C, valid, f"{case.name} bf16")
    # bf16 rows: the allowance of the cross-entropy head's test -- the round-to-nearest-even of the fp32 rows, bit for bit
    assert torch.equal(_bits(got["bf16"]["dl"]), _bits(got["f32"]["dl"].to(torch.bfloat16))), f"{case.name}: bf16 rows are not RNE(fp32 rows)"
    assert torch.equal(_bits(got["bf16"]["terms"]), _bits(got["f32"]["terms"]))


def test_no_gradient_asked_leaves_the_rest_alone(dev):
    case = next(c for c in S.CASES if c.spec == "ce_dice_ls" and c.shape == S.MEDIUM)
    v, y, valid, ref = S.case_reference(case)
    labels = v["lab"][case.kind].to(dev).contiguous()
    for lay in LAYOUTS:
        a = run_seg(dev, case.C, case.shape, v["x"], labels, case.kind, v["w"], S.spec_of(case.spec), lay, case.ld)
        b = run_seg(dev, case.C, case.shape, v["x"], labels, case.kind, v["w"], S.spec_of(case.spec), lay, case.ld, want_dl=False)
        assert torch.equal(_bits(a["terms"]), _bits(b["terms"])) and torch.equal(a["preds"], b["preds"]) and torch.equal(a["cm"], b["cm"])
        assert bool(torch.isnan(b["dl"].float()).all())


# ------------------------------------------------------------------------------------------------ exact cases
def _exact(dev, labels_i64, spec, layout, w=None):
    win = S.exact_winners()
    x = S.exact_logits(win, S.EXACT_C)
    return x, run_seg(dev, S.EXACT_C, S.EXACT_SHAPE, x, labels_i64.to(dev), "i64", w, spec, layout, 16)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_one_hot_softmax_on_its_labels_has_no_dice_loss_bit_for_bit(dev, layout):
    from flair_amd import SegLoss
    win = S.exact_winners()
    _, r = _exact(dev, win, SegLoss(ce=0.0, dice=1.0), layout)
    assert int(_bits(r["terms"]).ne(0).sum()) == 0, r["terms"]
    assert int(_bits(r["dl"]).ne(0).sum()) == 0, "a gradient element is not +0.0"
    assert torch.equal(r["preds"].long(), win.reshape(-1))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_pixel_ignored_has_no_dice_loss(dev, layout):
    from flair_amd import SegLoss
    win = S.exact_winners()
    _, r = _exact(dev, torch.full_like(win, 255), SegLoss(ce=0.0, dice=1.0, dice_smooth=1.0), layout)
    assert float(r["terms"][0]) == 0.0 and float(r["terms"][2]) == 0.0
    assert int(_bits(r["dl"]).ne(0).sum()) == 0
    assert int(r["cm"].abs().sum()) == 0


@pytest.mark.parametrize("name", ["dice", "dice_s1", "ce_dice_ls"])
def test_a_class_of_one_pixel_and_a_class_predicted_but_never_labelled(dev, name):
    win = S.exact_winners()
    lab = win.clone()
    a, b, other = 3, 5, 7
    assert int((win == a).sum()) > 1 and int((win == b).sum()) > 0
    ia = torch.nonzero(lab.flatten() == a).flatten()
    lab.view(-1)[ia[1:]] = other          # class a: one labelled pixel (predicted at several)
    lab[lab == b] = other                 # class b: predicted somewhere, never a label
    assert int((lab == a).sum()) == 1 and int((lab == b).sum()) == 0
    spec = S.spec_of(name)
    valid = torch.ones_like(lab, dtype=torch.bool)
    x = S.exact_logits(win, S.EXACT_C)
    ref = S.reference_of(x, lab, valid, None, spec)
    assert ref["dice"] > 0
    for layout in LAYOUTS:
        _, r = _exact(dev, lab, spec, layout)
        check_terms(r, ref, f"exact {name} {layout}")
        if layout != "bf16":
            check_dl(r["dl"], ref["dl"], S.EXACT_C, valid, f"exact {name} {layout}")


# ------------------------------------------------------------------------------------------------ determinism
def test_two_calls_give_the_same_bits_at_the_largest_shape(dev):
    case = next(c for c in S.CASES if c.shape == S.LARGE and "dice" in c.spec)
    v = K.case_values(*case.values)
    labels = v["lab"][case.kind].to(dev).contiguous()
    spec = S.spec_of(case.spec)
    for lay in ("nchw", "bf16"):
        a = run_seg(dev, case.C, case.shape, v["x"], labels, case.kind, v["w"], spec, lay, case.ld)
        b = run_seg(dev, case.C, case.shape, v["x"], labels, case.kind, v["w"], spec, lay, case.ld)
        assert torch.equal(_bits(a["terms"]), _bits(b["terms"])), lay
        assert torch.equal(_bits(a["dl"]), _bits(b["dl"])), lay


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_their_code_and_write_nothing(dev):
    L = CE._lib()
    l = L.lib()
    C, shape, ld = 13, S.SMALL, 16
    B, H, W = shape
    npix = B * H * W
    v = K.case_values(C, shape, "ints", "none")
    labels = v["lab"]["u8"].to(dev).contiguous()
    x = v["x"].to(dev).contiguous()
    rows = K.nhwc_rows(v["x"], 32).to(dev)
    good = _spec_c(S.spec_of("ce_dice_ls"))
    outs = {"terms": _Guarded(dev, 3, torch.float32, 7.0, guard=4), "preds": _Guarded(dev, npix, torch.uint8, 0xA5),
            "dl": _Guarded(dev, npix * 33, torch.float32, float("nan")), "cm": _Guarded(dev, 33 * 33, torch.int64, -7, guard=8),
            "ws": _Guarded(dev, l.flair_seg_loss_workspace_bytes(B, 33, H, W), torch.uint8, 0xC3)}

    def nchw(logits=L.ptr(x), lab=L.ptr(labels), kind=0, Cc=C, spec=good, terms=outs["terms"].ptr, dl=outs["dl"].ptr, ws=outs["ws"].ptr):
        sp = None if spec is None else ctypes.byref(spec)
        return l.flair_seg_loss(logits, lab, kind, None, B, Cc, H, W, sp, terms, dl, outs["preds"].ptr, None, None, outs["cm"].ptr, ws, L.stream())

    def nhwc(logits=L.ptr(rows), lab=L.ptr(labels), kind=0, Cc=C, ldv=ld, dtype=0, spec=good, terms=outs["terms"].ptr, dl=outs["dl"].ptr,
             ws=outs["ws"].ptr):
        sp = None if spec is None else ctypes.byref(spec)
        return l.flair_seg_loss_nhwc(logits, dtype, ldv, lab, kind, None, B, Cc, H, W, sp, terms, dl, outs["preds"].ptr, None,
                                     outs["cm"].ptr, ws, L.stream())

    bad_specs = [(-1, 0, 0, 0, 0, 1e-7), (0, 0, 0, 0, 0, 1e-7), (1, 1.0, 0, 0, 0, 1e-7), (1, 0, 0.5, 0, 0, 1e-7), (1, 0.1, 2, 0, 0, 1e-7),
                 (0, 0.1, 0, 1, 0, 1e-7), (0, 0, 2, 1, 0, 1e-7), (1, 0, 0, 1, -1, 1e-7), (1, 0, 0, 1, 0, 0.0), (1, 0, 0, -1, 0, 1e-7),
                 (float("nan"), 0, 0, 1, 0, 1e-7)]
    for vals in bad_specs:
        assert nchw(spec=_spec_c(vals)) == -20, vals
        assert nhwc(spec=_spec_c(vals)) == -20, vals
    assert b"flair_seg_loss_t" in l.flair_strerror(-20)
    assert nhwc(ldv=24, Cc=19) == -3 and nhwc(ldv=24) == -3 and nhwc(ldv=8, Cc=4) == -3 and nhwc(ldv=16, Cc=19) == -3
    assert nchw(Cc=33) == -2 and nhwc(Cc=33, ldv=32) == -2 and nchw(Cc=0) == -2
    assert nhwc(dtype=2) == -2
    for kw in (dict(logits=None), dict(lab=None), dict(spec=None), dict(terms=None), dict(ws=None), dict(kind=4), dict(kind=-1)):
        assert nchw(**kw) == -1, kw
        assert nhwc(**kw) == -1, kw
    assert nhwc(dl=outs["dl"].ptr + 4) == -3 and nhwc(logits=L.ptr(rows) + 4) == -3      # NHWC rows off their 16 bytes
    assert nchw(dl=outs["dl"].ptr + 2) == -3 and nchw(ws=outs["ws"].ptr + 2) == -3 and nhwc(ws=outs["ws"].ptr + 1) == -3
    torch.cuda.synchronize()
    for name, g in outs.items():
        assert torch.equal(_bits(g.full.cpu()), g.before), f"a refused call wrote to {name}"
    assert nchw() == 0 and nhwc() == 0      # the same arguments without the fault run


def test_ops_seg_loss_and_the_criterion_object(dev):
    """ops.seg_loss and head.FusedSegLoss: the reference's loss and gradient through autograd, last_preds and last_terms."""
    import flair_amd
    from flair_amd import ops
    case = next(c for c in S.CASES if c.spec == "ce_dice_ls" and c.shape == S.MEDIUM and c.kind == "i64")
    v, y, valid, ref = S.case_reference(case)
    spec = S.spec_of(case.spec)
    x = v["x"].to(dev)
    labels = v["lab"]["i64"].to(dev)
    cm = torch.zeros(case.C, case.C, dtype=torch.int64, device=dev)
    terms, dl, preds, tg = ops.seg_loss(x, labels, spec, v["w"].to(dev), want_preds="i64", confmat=cm, want_targets=True)
    check_terms({"terms": terms.cpu()}, ref, "ops.seg_loss")
    assert float((dl.cpu().double() - ref["dl"]).abs().max()) <= S.dl_bound(ref["dl"])
    ce_ref = v["int"]
    assert torch.equal(preds.cpu(), ce_ref["preds"]) and np.array_equal(cm.cpu().numpy(), ce_ref["confmat"])
    crit = flair_amd.FusedSegLoss(spec, weight=v["w"]).to(dev)
    xr = x.clone().requires_grad_(True)
    loss = crit(xr, labels)
    (2.0 * loss).backward()
    assert abs(float(loss.detach()) - ref["loss"]) <= S.loss_bound(ref["loss"])
    assert float((xr.grad.cpu().double() - 2.0 * ref["dl"]).abs().max()) <= 2.0 * S.dl_bound(ref["dl"])
    assert torch.equal(crit.last_preds.cpu(), ce_ref["preds"]) and torch.equal(_bits(crit.last_terms.cpu()), _bits(terms.cpu()))
    assert "SegLoss(" in repr(crit)


# ------------------------------------------------------------------------------------------------ the trainer
TRAINER_SPECS = {"ce_dice_ls": dict(ce=1.0, dice=1.0, label_smoothing=0.1), "focal2": dict(focal_gamma=2.0)}
LR = 0.02


def _model(dev, C, seed=5):
    import flair_amd
    from oracle import unet_resnet34 as om
    hip = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=C, compute_dtype="f32")
    hip.load_state_dict(om.seeded_model(5, C, seed).state_dict(), strict=True)
    return hip.to(dev).train()


def _batch(dev, C, seed=4):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, 5, 64, 64, generator=g)
    lab = torch.randint(0, C, (2, 64, 64), generator=g)
    lab[0, :4, :9] = 255                      # some ignored pixels
    return x.to(dev), lab.to(torch.uint8).to(dev), torch.linspace(0.5, 2, C)


def _torch_objective(logits, lab, w, spec):
    """The objective in plain torch operations on the logits' device, in their dtype (seg_loss_cases.terms_torch)."""
    y = lab.long()
    valid = y < logits.shape[1]
    ce, dice = S.terms_torch(logits, y, valid, w, spec)
    return spec.ce * ce + spec.dice * dice


_D_CE = {}


def _d_ce(dev, C):
    """The deviation of the flat weights between SegTrainer(loss=None).train_step and a twin stepping through autograd with
    F.cross_entropy and torch.optim.SGD: code that was there before against torch.  Measured on an MI355X: 5.96e-8 at C = 13 and
    1.19e-7 at C = 19 (one or two units in the last place of a weight near 1), so the trainer bound max(1e-7, 4 d_CE) is 2.4e-7
    and 4.8e-7; the trainer with a specification measured 1.19e-7 against the torch twin at both class counts and for both
    specifications, and 0 against the criterion twin."""
    if C not in _D_CE:
        import flair_amd
        a, b = _model(dev, C), _model(dev, C)
        x, lab, w = _batch(dev, C)
        flair_amd.SegTrainer(a, lr=LR, class_weight=w).train_step(x, lab)
        tgt = torch.where(lab < C, lab.long(), torch.full_like(lab.long(), -100))
        F.cross_entropy(b(x), tgt, weight=w.to(dev), ignore_index=-100).backward()
        torch.optim.SGD(b.parameters(), lr=LR).step()
        _D_CE[C] = float((a.flat_parameters() - b.flat_parameters()).abs().max())
        print(f"d_CE at C = {C}: {_D_CE[C]:.3e}")
    return _D_CE[C]


@pytest.mark.parametrize("name", list(TRAINER_SPECS))
@pytest.mark.parametrize("C", [13, 19])
def test_trainer_step_matches_autograd_twins(dev, C, name):
    import flair_amd
    spec = flair_amd.SegLoss(**TRAINER_SPECS[name])
    bound = max(1e-7, 4 * _d_ce(dev, C))
    a, b, c = _model(dev, C), _model(dev, C), _model(dev, C)
    x, lab, w = _batch(dev, C)
    tr = flair_amd.SegTrainer(a, lr=LR, class_weight=w, loss=spec)
    la = tr.train_step(x, lab)
    assert la.data_ptr() == tr.loss_terms.data_ptr() and tr.loss_terms.shape == (3,)
    # twin 1: the objective in plain torch operations, autograd, torch.optim.SGD
    logits = b(x)
    lb = _torch_objective(logits, lab, w, spec)
    lb.backward()
    torch.optim.SGD(b.parameters(), lr=LR).step()
    # twin 2: the criterion object on the autograd surface
    crit = flair_amd.FusedSegLoss(spec, weight=w).to(dev)
    lc = crit(c(x), lab)
    lc.backward()
    torch.optim.SGD(c.parameters(), lr=LR).step()
    ref64 = S.reference_of(logits.detach().cpu(), lab.cpu().long(), lab.cpu() < C, w, spec)
    dev_b = float((a.flat_parameters() - b.flat_parameters()).abs().max())
    dev_c = float((a.flat_parameters() - c.flat_parameters()).abs().max())
    print(f"C {C} {name}: loss {float(la):.7f} torch {float(lb):.7f} criterion {float(lc):.7f} fp64 {ref64['loss']:.7f}; "
          f"weights vs torch twin {dev_b:.2e}, vs criterion twin {dev_c:.2e} (bound {bound:.1e})")
    for got in (float(la), float(lc)):
        assert abs(got - ref64["loss"]) <= S.loss_bound(ref64["loss"])
    assert abs(float(la) - float(lb)) <= S.loss_bound(ref64["loss"])
    check_terms({"terms": tr.loss_terms.cpu()}, ref64, f"trainer C {C} {name}")
    assert dev_b <= bound and dev_c <= bound
    # predictions: the twin's argmax wherever its two largest probabilities are apart
    top = torch.softmax(logits.detach().double(), 1).topk(2, 1).values
    clear = (top[:, 0] - top[:, 1]) > 1e-5
    assert float(clear.float().mean()) > 0.99
    assert torch.equal(tr._preds[clear].long(), logits.detach().argmax(1)[clear])
    assert torch.equal(tr._preds, crit.last_preds.to(torch.uint8))
    assert int(tr.confmat.sum()) == int((lab < C).sum())


@pytest.mark.parametrize("C", [13, 19])
def test_validate_step_accumulates_the_objective(dev, C):
    import flair_amd
    spec = flair_amd.SegLoss(**TRAINER_SPECS["ce_dice_ls"])
    a, b = _model(dev, C), _model(dev, C)
    x, lab, w = _batch(dev, C)
    x2, lab2, _ = _batch(dev, C, seed=9)
    tr = flair_amd.SegTrainer(a, lr=LR, class_weight=w, loss=spec, class_names=[f"k{i}" for i in range(C)])
    before = a.flat_parameters().clone()
    from oracle import unet_resnet34 as om
    oracle = om.seeded_model(5, C, 5).eval()      # the weights _model loads
    want, got, twins = [], [], []
    for xx, ll in ((x, lab), (x2, lab2)):
        got.append(float(tr.validate_step(xx, ll)))
        logits = b.eval_logits(xx).cpu()       # the twin in eval mode
        ref = S.reference_of(logits, ll.cpu().long(), ll.cpu() < C, w, spec)
        want.append(ref["loss"])
        assert abs(got[-1] - want[-1]) <= S.loss_bound(want[-1]), (got, want)
        # the torch twin in eval mode: the oracle model on the CPU and the objective in plain torch operations, nothing of it native.
        # The project's fp32 bar for the eval forward is logits within 1e-3 (test_gpu_validate.py); log-softmax moves by at most twice
        # that, so CE by 2e-3, and a probability by the relative 2e-3, so each Dice ratio (2 I + s) / (P + T + s) <= 1 by at most 4e-3
        with torch.no_grad():
            twin = float(_torch_objective(oracle(xx.cpu()), ll.cpu(), w, spec))
        print(f"C {C}: validate_step {got[-1]:.7f} native logits + fp64 {want[-1]:.7f} torch twin {twin:.7f}")
        assert abs(got[-1] - twin) <= spec.ce * 2e-3 + spec.dice * 4e-3, (got[-1], twin)
        twins.append(twin)
    plain = flair_amd.SegTrainer(b, lr=LR, class_weight=w)
    assert abs(float(plain.validate_step(x, lab)) - got[0]) > 1e-3, "the objective is not the plain cross entropy's"
    out = tr.validation_epoch_end()
    mean = sum(want) / 2
    assert abs(float(out["val_loss"]) - mean) <= S.loss_bound(mean)
    assert abs(float(out["val_loss"]) - sum(twins) / 2) <= spec.ce * 2e-3 + spec.dice * 4e-3
    assert 0.0 <= float(out["val_miou"]) <= 1.0 and out["val_iou"].shape == (C,)
    assert torch.equal(a.flat_parameters(), before)


def test_fused_step_takes_the_criterions_objective(dev):
    """The Lightning surface: a criterion that carries a SegLoss is computed as that objective, not silently as plain CE."""
    import flair_amd
    from flair_amd.task_module import fused_step
    case = next(c for c in S.CASES if c.spec == "ce_dice_ls" and c.kind == "onehot")
    v, y, valid, ref = S.case_reference(case)
    x = v["x"].to(dev).requires_grad_(True)
    msk = v["lab"]["onehot"].to(dev)
    crit = flair_amd.FusedSegLoss(S.spec_of(case.spec), weight=v["w"])
    loss, preds, targets = fused_step(x, msk, crit)
    plain, preds_ce, targets_ce = fused_step(x.detach(), msk, flair_amd.FusedCrossEntropyLoss(weight=v["w"]))
    assert abs(float(loss.detach()) - ref["loss"]) <= S.loss_bound(ref["loss"])
    assert abs(float(plain) - v["onehot"]["loss"]) <= K.loss_bound(v["onehot"]["loss"])
    assert abs(float(loss.detach()) - float(plain)) > 0.1
    assert torch.equal(preds, preds_ce) and torch.equal(targets, targets_ce)
    loss.backward()
    assert float((x.grad.cpu().double() - ref["dl"]).abs().max()) <= S.dl_bound(ref["dl"])


def test_defaults_never_reach_the_new_entry_points(dev, monkeypatch):
    import flair_amd
    from flair_amd import _lib as L
    from flair_amd.task_module import fused_step
    l = L.lib()
    calls = []
    for name in ("flair_seg_loss", "flair_seg_loss_nhwc"):
        real = getattr(l, name)

        def counted(*a, _real=real, _name=name):
            calls.append(_name)
            return _real(*a)
        monkeypatch.setattr(l, name, counted)
    C = 13
    m = _model(dev, C)
    x, lab, w = _batch(dev, C)
    tr = flair_amd.SegTrainer(m, lr=LR, class_weight=w)
    assert tr.loss_terms is None and tr.loss_spec is None
    tr.train_step(x, lab)
    tr.validate_step(x, lab)
    tr.validation_epoch_end()
    logits = torch.randn(2, C, 8, 8, device=dev)
    fused_step(logits, lab[:, :8, :8].contiguous(), flair_amd.FusedCrossEntropyLoss(weight=w))
    flair_amd.FusedCrossEntropyLoss()(logits, lab[:, :8, :8].long())
    assert calls == []
    # and the wrapper does see the calls of a trainer with a specification
    tr2 = flair_amd.SegTrainer(m, lr=LR, class_weight=w, loss=flair_amd.SegLoss(dice=1.0))
    tr2.train_step(x, lab)
    tr2.validate_step(x, lab)
    assert calls == ["flair_seg_loss_nhwc", "flair_seg_loss"]
    with pytest.raises(TypeError):
        flair_amd.SegTrainer(m, lr=LR, loss={"dice": 1.0})
