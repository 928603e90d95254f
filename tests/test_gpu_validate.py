"""SegTrainer.validate_step / validation_epoch_end on the GPU: the per-pixel head of the reference's step() (label argmax, weighted
cross-entropy mean, argmax(softmax), confusion-matrix bincount; task_module.py:71-79, 104-154) taken out of the head convolution's
register epilogue (the ce_ fields of flair_unet_fwd_opts_t), and the fallback that runs the head convolution and flair_ce_head_nhwc's kernels instead.

Loss tolerance, used by every loss assertion against the HIP logits: "truth" is the fp64 host recomputation of the weighted CE mean
(oracle.seg_step.cross_entropy_np) from the fp32 NCHW logits the same eval forward returns — the rounded values the epilogue sees —
and the yardstick is flair_ce_head_nhwc on that forward:  |new - truth| <= |old - truth| + 64 * 2^-24 * |truth|.  The added term
covers what differs between the two kernels at these shapes: at most 12 sequential fp32 adds per lane (three tiles of four pixel
blocks, one pixel per lane and block), 8 reduction levels over 256 threads, and a three-term reordering of the exp-sum; both share
__expf / logf.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LOSS_SLACK = 64 * 2.0 ** -24


def _pair(in_ch, classes, seed, dev, dtype="f32"):
    """Oracle model (CPU) and the HIP model loaded with the same seeded weights."""
    import flair_amd
    from oracle import unet_resnet34 as om
    ref = om.seeded_model(in_ch, classes, seed)
    hip = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=in_ch, classes=classes, compute_dtype=dtype)
    hip.load_state_dict(ref.state_dict(), strict=True)
    return ref, hip.to(dev)


def _tune(key, value):
    from flair_amd import _lib as L
    L.check(L.lib().flair_tune_set(key, value), "flair_tune_set")


class _head_ce:
    """FLAIR_HEAD_CE = value inside the block; the library's default (0: the fallback, profiles/validate_step.json) behind it."""
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        _tune(b"FLAIR_HEAD_CE", self.value)

    def __exit__(self, *exc):
        _tune(b"FLAIR_HEAD_CE", 0)


@pytest.fixture(params=[1, 0], ids=["fused", "fallback"])
def head_ce(request):
    with _head_ce(request.param):
        yield request.param


def _weights(C):
    w = torch.linspace(0.5, 2, C)
    w[1] = 0.0
    w[C - 2] = 0.0
    return w


def _labels(shape, C, seed, absent=3, ignored=0.1):
    """uint8 labels: every class but `absent`, about `ignored` of the pixels set to 255."""
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, C - 1, shape, generator=g)
    lab = torch.where(lab >= absent, lab + 1, lab)
    lab[torch.rand(shape, generator=g) < ignored] = 255
    return lab.to(torch.uint8)


def _old_head(m, x, lab, w, dev):
    """flair_ce_head_nhwc over the NHWC logits of one eval forward of `m` (the path train_step uses), and the fp32 NCHW logits."""
    from flair_amd import _lib as L
    from flair_amd import ops
    l = L.lib()
    B, _, H, W = x.shape
    C = m.classes
    logits = m._c_forward(x, training=False, want_logits=True)
    m._c_forward(x, training=False, want_logits=False)
    h = m._hh(False)
    nhwc = l.flair_unet_logits_nhwc(h)
    assert nhwc
    loss = torch.empty((), dtype=torch.float32, device=dev)
    preds = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
    cm = torch.zeros(C, C, dtype=torch.int64, device=dev)
    ws = torch.empty(l.flair_ce_workspace_bytes(B, H, W) + 256, dtype=torch.uint8, device=dev)
    kind = 3 if lab.dtype == torch.float32 else ops._LABEL_KIND[lab.dtype]
    L.check(l.flair_ce_head_nhwc(nhwc, m._dt, l.flair_unet_head_ld(m._h), L.ptr(lab), kind, L.ptr(w), B, C, H, W, L.ptr(loss), None,
                                 L.ptr(preds), None, L.ptr(cm), L.ptr(ws), L.stream()), "ce_head_nhwc")
    return logits, loss, preds, cm


def _truth(logits, lab, w):
    """fp64 weighted CE mean over the valid pixels of fp32 NCHW logits."""
    from oracle import seg_step
    C = logits.shape[1]
    lg = logits.detach().cpu().numpy().astype(np.float64).transpose(0, 2, 3, 1).reshape(-1, C)
    lb = lab.cpu().numpy().reshape(-1).astype(np.int64)
    ok = lb < C
    loss, _ = seg_step.cross_entropy_np(lg[ok].T[None, :, :, None], lb[ok][None, :, None], w.numpy().astype(np.float64))
    return float(loss)


@pytest.fixture(scope="module")
def cases(dev):
    """case(dtype, classes, shape) -> model, trainer, inputs and references of that case: built once per module, shared by the tests
    below (each of which starts from reset accumulators), never modified, freed with the module."""
    import flair_amd
    built = {}

    def case(dtype, C, shape):
        key = (dtype, C, shape)
        if key not in built:
            _, m = _pair(5, C, 23, dev, dtype)
            m = m.eval()
            g = torch.Generator().manual_seed(5)
            x = torch.randn(*shape, generator=g).to(dev)
            lab = _labels((shape[0], shape[2], shape[3]), C, 6).to(dev)
            w = _weights(C)
            tr = flair_amd.SegTrainer(m, lr=0.0, class_weight=w)
            logits, old_loss, _, _ = _old_head(m, x, lab, tr.class_weight, dev)
            truth = _truth(logits, lab, w)
            built[key] = dict(m=m, tr=tr, x=x, lab=lab, w=w, truth=truth, old=old_loss.item())
        return built[key]

    yield case
    built.clear()
    torch.cuda.empty_cache()


def _assert_loss(new, c, what):
    e_new, e_old = abs(new - c["truth"]), abs(c["old"] - c["truth"])
    print(f"{what}: loss {new!r} truth {c['truth']!r} |new-truth| {e_new:.3e} |old-truth| {e_old:.3e} "
          f"slack {LOSS_SLACK * abs(c['truth']):.3e}")
    assert e_new <= e_old + LOSS_SLACK * abs(c["truth"]), (new, c["old"], c["truth"])


def _validate_and_check(c, C, what):
    """One validate_step on fresh accumulators against predict, the host confusion matrix and the loss tolerance; a second identical
    call must return the same bits and double the matrix.  Returns (loss, preds, confusion matrix of one call)."""
    from oracle import seg_step
    tr, x, lab = c["tr"], c["x"], c["lab"]
    tr.validation_epoch_end()   # whatever an earlier test left in the shared trainer's accumulators
    loss = tr.validate_step(x, lab)
    preds, cm = tr._val_preds.clone(), tr.val_confmat.clone()
    assert preds.dtype == torch.uint8 and preds.shape == lab.shape
    ref_preds = tr.predict(x)
    assert torch.equal(preds, ref_preds), int((preds != ref_preds).sum())
    lb, pr = lab.cpu().numpy(), preds.cpu().numpy()
    ok = lb != 255
    cm_ref = seg_step.confusion_matrix_np(lb[ok], pr[ok], C)
    assert cm_ref[3].sum() == 0 and cm_ref.sum() == ok.sum()
    assert np.array_equal(cm.cpu().numpy(), cm_ref)
    _assert_loss(loss.item(), c, what)
    loss2 = tr.validate_step(x, lab)
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)), (loss.item(), loss2.item())
    assert torch.equal(tr.val_confmat, 2 * cm)
    tr.validation_epoch_end()   # leave the shared trainer's accumulators empty
    return loss, preds, cm


ONE_TILE = (3, 5, 96, 160)


@pytest.mark.parametrize("dtype,C", [("f32", 13), ("f32", 19), ("bf16", 13), ("bf16", 19)])
def test_validate_step_one_tile_per_workgroup(dev, cases, dtype, C):
    """180 tiles, one per workgroup; 13 classes sit in one 16-wide column block, 19 in a 32-wide one (eight channels per lane)."""
    from flair_amd import _lib as L
    c = cases(dtype, C, ONE_TILE)
    with _head_ce(1):
        _validate_and_check(c, C, f"one tile {dtype} C={C}")
        assert not L.lib().flair_unet_logits_nhwc(c["m"]._hh(False))   # the fused flavour ran: no logits were kept


@pytest.mark.parametrize("dtype,C", [("bf16", 19), ("f32", 13)])
def test_validate_step_persistent_loop_wraps_both_halo_slots(dev, cases, dtype, C):
    """FLAIR_HALO_P_WGS=1: 256 workgroups for 600 tiles — 88 of them walk three tiles (slot A, slot B, slot A again), the rest two;
    the per-lane loss accumulator and the LDS histogram live across the whole loop."""
    from flair_amd import _lib as L
    _tune(b"FLAIR_HALO_P_WGS", 1)
    try:
        c = cases(dtype, C, (5, 5, 160, 192))
        with _head_ce(1):
            _validate_and_check(c, C, f"wrap {dtype} C={C}")
            assert not L.lib().flair_unet_logits_nhwc(c["m"]._hh(False))
    finally:
        _tune(b"FLAIR_HALO_P_WGS", 0)


@pytest.mark.parametrize("dtype,C", [("f32", 13), ("f32", 19), ("bf16", 13), ("bf16", 19)])
def test_fallback_equals_fused(dev, cases, dtype, C):
    """FLAIR_HEAD_CE=0: the same request runs the head convolution to NHWC logits and ce_head on them inside the executor."""
    from flair_amd import _lib as L
    c = cases(dtype, C, ONE_TILE)
    h = c["m"]._hh(False)
    with _head_ce(0):
        loss_b, preds_b, cm_b = _validate_and_check(c, C, f"fallback {dtype} C={C}")
        assert L.lib().flair_unet_logits_nhwc(h)
    with _head_ce(1):
        loss_f, preds_f, cm_f = _validate_and_check(c, C, f"fused {dtype} C={C}")
        assert not L.lib().flair_unet_logits_nhwc(h)
    assert torch.equal(preds_b, preds_f) and torch.equal(cm_b, cm_f)


def test_label_kinds_give_identical_results(dev, head_ce):
    import flair_amd
    C = 13
    _, m = _pair(5, C, 11, dev)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(2, 5, 64, 64, generator=g).to(dev)
    lab = torch.randint(0, C, (2, 64, 64), generator=g)
    w = _weights(C)
    tr = flair_amd.SegTrainer(m.eval(), lr=0.0, class_weight=w)
    onehot = torch.nn.functional.one_hot(lab, C).permute(0, 3, 1, 2).contiguous().float()
    res = []
    for labels in (lab.to(torch.uint8), lab.to(torch.int32), lab.to(torch.int64), onehot):
        tr.val_confmat.zero_()
        loss = tr.validate_step(x, labels.to(dev))
        res.append((loss.clone(), tr._val_preds.clone(), tr.val_confmat.clone()))
    for loss, preds, cm in res[1:]:
        assert torch.equal(loss.view(torch.int32), res[0][0].view(torch.int32))
        assert torch.equal(preds, res[0][1]) and torch.equal(cm, res[0][2])
    assert int(res[0][2].sum()) == lab.numel()
    # nothing valid: 0 / 0, like flair_ce_head_nhwc
    ignored = torch.full((2, 64, 64), 255, dtype=torch.uint8, device=dev)
    tr.val_confmat.zero_()
    loss = tr.validate_step(x, ignored)
    _, old_loss, old_preds, old_cm = _old_head(m, x, ignored, tr.class_weight, dev)
    print("all ignored:", loss.item(), old_loss.item())
    assert (torch.isnan(loss) and torch.isnan(old_loss)) or loss.item() == old_loss.item()
    assert torch.equal(tr._val_preds, old_preds) and torch.equal(tr.val_confmat, old_cm) and int(old_cm.sum()) == 0


def test_validation_leaves_training_alone(dev, head_ce):
    import flair_amd
    C = 13
    _, a = _pair(5, C, 5, dev)
    _, b = _pair(5, C, 5, dev)
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(2, 5, 64, 64, generator=g).to(dev) for _ in range(3)]
    labs = [torch.randint(0, C, (2, 64, 64), generator=g).to(torch.uint8).to(dev) for _ in range(3)]
    w = torch.linspace(0.5, 2, C)
    ta = flair_amd.SegTrainer(a.train(), lr=0.02, class_weight=w)
    tb = flair_amd.SegTrainer(b.train(), lr=0.02, class_weight=w)
    la0 = ta.train_step(xs[0], labs[0]).item()
    before = (a.flat_parameters().clone(), a.flat_buffers().clone(), a._flat_n.clone())
    ta.validate_step(xs[2], labs[2])
    assert all(torch.equal(u, v) for u, v in zip(before, (a.flat_parameters(), a.flat_buffers(), a._flat_n)))
    la1 = ta.train_step(xs[1], labs[1]).item()
    lb0 = tb.train_step(xs[0], labs[0]).item()
    lb1 = tb.train_step(xs[1], labs[1]).item()
    assert (la0, la1) == (lb0, lb1)
    assert torch.equal(a.flat_parameters(), b.flat_parameters())
    assert torch.equal(a.flat_buffers(), b.flat_buffers())
    nbt = lambda m: [v.item() for k, v in m.state_dict().items() if k.endswith("num_batches_tracked")]
    assert nbt(a) == nbt(b) and len(nbt(a)) > 0
    # the running statistics are used whatever the module's mode says
    l_train = ta.validate_step(xs[2], labs[2]).clone()
    a.eval()
    l_eval = ta.validate_step(xs[2], labs[2])
    assert torch.equal(l_train.view(torch.int32), l_eval.view(torch.int32))


def test_validation_epoch_end(dev, head_ce):
    import flair_amd
    from oracle import seg_step
    C = 13
    _, m = _pair(5, C, 7, dev)
    g = torch.Generator().manual_seed(9)
    w = _weights(C)
    names = [f"class_{i}" for i in range(C)]
    tr = flair_amd.SegTrainer(m.eval(), lr=0.0, class_weight=w, class_names=names)
    losses, cm = [], np.zeros((C, C), np.int64)
    for i in range(2):
        x = torch.randn(2, 5, 64, 64, generator=g).to(dev)
        lab = _labels((2, 64, 64), C, 20 + i)
        losses.append(tr.validate_step(x, lab.to(dev)))
        lb, pr = lab.numpy(), tr._val_preds.cpu().numpy()
        cm += seg_step.confusion_matrix_np(lb[lb != 255], pr[lb != 255], C)
    assert not torch.equal(losses[0], losses[1])
    out = tr.validation_epoch_end()
    mean = (np.float64(losses[0].item()) + np.float64(losses[1].item())) / 2
    assert abs(out["val_loss"].item() - mean) <= 2.0 ** -24 * abs(mean)   # fp64 sum of two fp32 values, rounded to fp32 once
    # the tolerance of the project's Jaccard assertions (fp32 outputs of an fp64 computation)
    assert abs(out["val_miou"].item() - seg_step.jaccard_from_confmat(cm, "weighted")) < 1e-6
    assert np.allclose(out["val_iou"].cpu().numpy(), seg_step.jaccard_from_confmat(cm, None), atol=1e-6)
    assert set(out["val_iou_named"]) == {names[i] for i in range(C) if w[i] != 0} and len(out["val_iou_named"]) == C - 2
    assert all(abs(out["val_iou_named"][names[i]] - out["val_iou"][i].item()) == 0 for i in range(C) if w[i] != 0)
    # reset: the next epoch starts from nothing
    assert int(tr.val_confmat.sum()) == 0 and tr.val_loss_sum.item() == 0 and tr.val_count.item() == 0
    empty = tr.validation_epoch_end()
    assert torch.isnan(empty["val_loss"]) and empty["val_miou"].item() == 0 and float(empty["val_iou"].abs().sum()) == 0
    # without names the classes go by index
    tr2 = flair_amd.SegTrainer(m, lr=0.0, class_weight=w)
    assert set(tr2.validation_epoch_end()["val_iou_named"]) == {i for i in range(C) if w[i] != 0}


@pytest.mark.parametrize("C", [13, 19])
def test_validate_step_against_the_oracle(dev, C, head_ce):
    """ref.eval() on the CPU + oracle.seg_step.step_torch: the project's fp32 bar (logits within 1e-3, so the loss within 2e-3) and
    identical predictions wherever the oracle's top-2 logit gap exceeds 2e-3."""
    import flair_amd
    from oracle import seg_step
    ref, m = _pair(5, C, 17, dev)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 64, 64, generator=g)
    lab = torch.randint(0, C, (2, 64, 64), generator=g)
    onehot = torch.nn.functional.one_hot(lab, C).permute(0, 3, 1, 2).contiguous().float()
    w = torch.linspace(0.5, 2, C)
    with torch.no_grad():
        logits = ref.eval()(x)
        loss_ref, preds_ref, _ = seg_step.step_torch(logits, onehot, w)
    tr = flair_amd.SegTrainer(m.train(), lr=0.0, class_weight=w)
    loss = tr.validate_step(x.to(dev), onehot.to(dev)).item()
    print("oracle:", loss_ref.item(), "hip:", loss)
    assert abs(loss - loss_ref.item()) <= 2e-3
    top2 = logits.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2e-3
    preds = tr._val_preds.cpu().to(torch.int64)
    assert sure.float().mean() > 0.9
    assert torch.equal(preds[sure], preds_ref.view(2, 64, 64)[sure])


def test_conflicting_requests_are_refused_and_dropped(dev):
    from flair_amd import _lib as L
    C = 13
    _, m = _pair(5, C, 13, dev)
    _, untouched = _pair(5, C, 13, dev)
    m, untouched = m.eval(), untouched.eval()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 5, 64, 64, generator=g).to(dev)
    lab = torch.zeros(1, 64, 64, dtype=torch.uint8, device=dev)
    m._c_forward(x, training=False)   # flat parameters, eval handle and workspace exist
    l = L.lib()
    h = m._hh(False)
    ws = m._workspace(1, 64, 64, False)
    loss = torch.full((), 7.0, dtype=torch.float32, device=dev)
    preds = torch.full((1, 64, 64), 99, dtype=torch.uint8, device=dev)
    cews = torch.empty(l.flair_ce_workspace_bytes(1, 64, 64) + 256, dtype=torch.uint8, device=dev)
    ce = dict(ce_labels=L.ptr(lab), ce_label_kind=0, ce_loss=L.ptr(loss), ce_workspace=L.ptr(cews))

    def fwd(handle, training, arena, **fields):
        opts = L.UnetFwdOpts(**fields)
        with torch.cuda.device(dev):
            return l.flair_unet_forward(handle, L.ptr(m._flat_p), L.ptr(m._flat_b), L.ptr(x), None, 1, 64, 64, training, L.ptr(arena),
                                        arena.numel(), L.stream(), ctypes.byref(opts))

    rc = fwd(h, 0, ws, preds_u8=L.ptr(preds), **ce)
    assert rc == -15 and b"ce_labels" in l.flair_strerror(rc)
    assert loss.item() == 7.0 and int((preds != 99).sum()) == 0   # nothing ran
    # malformed structs are refused before that: no loss, no workspace, a label kind out of range, a probability map without preds
    for bad in (dict(ce, ce_loss=None), dict(ce, ce_workspace=None), dict(ce, ce_label_kind=4), dict(ce, ce_label_kind=-1),
                dict(maxprob_f32=L.ptr(loss))):
        assert fwd(h, 0, ws, **bad) == -1
    assert loss.item() == 7.0 and int((preds != 99).sum()) == 0
    # nothing is kept: a plain eval forward behaves like an untouched model's
    assert torch.equal(m._c_forward(x, training=False), untouched._c_forward(x, training=False))
    assert loss.item() == 7.0 and int((preds != 99).sum()) == 0
    # the CE head on a training forward is refused as well
    wst = m._workspace(1, 64, 64, True)
    rc = fwd(m._h, 1, wst, **ce)
    assert rc == -15 and loss.item() == 7.0
