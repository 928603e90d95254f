"""Metadata fusion in the native eval forward (rows_f32 of flair_unet_fwd_opts_t): the row-vector add of model.py:59-60 on the executor's own NHWC
bottleneck, between the encoder and the decoder of ONE flair_unet_forward, reachable from Unet (eval_logits / predict_classes),
FLAIR_ModelFactory, segmentation_task_predict.predict_step and SegTrainer (validate_step / predict).

Why bit equality with the split path (encoder, flair_add_rowvec_nchw, decoder, head as three native calls) is the bar: in eval mode
every unit materialises its output and both paths launch the same kernels on the same values.  The split path's boundary crossings
(feature -> fp32 NCHW -> feature) are exact in both compute dtypes (bf16 -> fp32 -> bf16 loses nothing), and the bottleneck plus
rows is one fp32 add rounded once by the same conversion on either side.  The premise — plain fused forward == plain split path —
is asserted next to every such comparison.
"""
import os

import numpy as np
import pytest
import torch

import metadata_eval_cases as mc

pytestmark = pytest.mark.gpu

CLASSES19 = {1: [1, 'building'], 2: [1, 'pervious surface'], 3: [1, 'impervious surface'], 4: [1, 'bare soil'],
             5: [1, 'water'], 6: [1, 'coniferous'], 7: [1, 'deciduous'], 8: [1, 'brushwood'], 9: [1, 'vineyard'],
             10: [1, 'herbaceous vegetation'], 11: [1, 'agricultural land'], 12: [1, 'plowed land'],
             13: [1, 'swimming_pool'], 14: [1, 'snow'], 15: [0, 'clear cut'], 16: [0, 'mixed'], 17: [0, 'ligneous'],
             18: [1, 'greenhouse'], 19: [0, 'other']}

SMALL = (2, 5, 96, 160)   # bottleneck 3 rows x 5 columns


def _config(n_ch, classes, use_metadata=False):
    return {"model_framework": {"model_provider": "SegmentationModelsPytorch",
                                "SegmentationModelsPytorch": {"encoder_decoder": "resnet34_unet", "encoder_weights": None}},
            "use_metadata": use_metadata, "channels": list(range(1, n_ch + 1)), "classes": classes}


def _pair(in_ch, classes, seed, dev, dtype="f32"):
    import flair_amd
    from oracle import unet_resnet34 as om
    ref = om.seeded_model(in_ch, classes, seed)
    hip = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=in_ch, classes=classes, compute_dtype=dtype)
    hip.load_state_dict(ref.state_dict(), strict=True)
    return ref, hip.to(dev)


class _env:
    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        self.old = os.environ.get(self.key)
        os.environ[self.key] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(self.key, None)
        else:
            os.environ[self.key] = self.old


def _add_nhwc(x, v):
    from flair_amd import _lib as L
    N, H, W, C = x.shape
    return L.lib().flair_add_rowvec_nhwc(L.dtype_code(x.dtype), L.ptr(x), L.ptr(v), N, H, W, C, L.stream())


def _split(m, x, v=None):
    """The eval-mode split path of FLAIR_ModelFactory.forward: encoder, flair_add_rowvec_nchw on feats[-1], decoder, head."""
    from flair_amd import _lib as L
    feats = m._c_encoder_forward(x, training=False)
    if v is not None:
        N, C, H, W = feats[-1].shape
        L.check(L.lib().flair_add_rowvec_nchw(L.ptr(feats[-1]), L.ptr(v), N, C, H, W, L.stream()), "add_rowvec_nchw")
    return m._c_head_forward(m._c_decoder_forward(feats, training=False), training=False)


# ------------------------------------------------------------------------------------------------ 1. operator
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_add_rowvec_nhwc_bits(dev, dtype):
    x, v, want = mc.case(dtype)
    xd, vd = x.to(dev), v.to(dev)
    assert _add_nhwc(xd, vd) == 0
    assert torch.equal(xd.cpu(), want), int((xd.cpu() != want).sum())


def test_add_rowvec_nhwc_equals_the_nchw_kernel_at_the_bottleneck_shape(dev):
    from flair_amd import _lib as L
    x, v = mc.wide_case()
    xd, vd = x.to(dev), v.to(dev)
    nchw = xd.permute(0, 3, 1, 2).contiguous()
    L.check(L.lib().flair_add_rowvec_nchw(L.ptr(nchw), L.ptr(vd), 2, 512, 16, 16, L.stream()), "add_rowvec_nchw")
    assert _add_nhwc(xd, vd) == 0
    assert torch.equal(xd.permute(0, 3, 1, 2), nchw)
    assert not torch.equal(xd.cpu(), x)


def test_add_rowvec_nhwc_refuses_bad_channel_counts_and_alignment(dev):
    from flair_amd import _lib as L
    l = L.lib()
    x = torch.zeros(1, 2, 2, 32, device=dev)
    v = torch.zeros(1, 2, device=dev)
    before = x.clone()
    for C in (4, 12, 20):
        assert l.flair_add_rowvec_nhwc(0, L.ptr(x), L.ptr(v), 1, 2, 2, C, L.stream()) == -2
    assert l.flair_add_rowvec_nhwc(0, x.data_ptr() + 4, L.ptr(v), 1, 2, 2, 8, L.stream()) == -2
    assert l.flair_add_rowvec_nhwc(2, L.ptr(x), L.ptr(v), 1, 2, 2, 8, L.stream()) == -2
    assert l.flair_add_rowvec_nhwc(0, None, L.ptr(v), 1, 2, 2, 8, L.stream()) == -1
    assert torch.equal(x, before)


# ------------------------------------------------------------------------------------------------ 2. small executor
@pytest.fixture(scope="module")
def small(dev):
    """case(dtype) -> eval model (13 classes, seeded), input, rows and the plain fused logits: built once, never modified."""
    built = {}

    def case(dtype):
        if dtype not in built:
            _, m = _pair(5, 13, 31, dev, dtype)
            m = m.eval()
            g = torch.Generator().manual_seed(12)
            x = torch.randn(*SMALL, generator=g).to(dev)
            v = torch.randn(2, 3, generator=g).to(dev)
            plain = m._c_forward(x, training=False).clone()
            built[dtype] = dict(m=m, x=x, v=v, plain=plain)
        return built[dtype]

    yield case
    built.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_fused_rows_equal_the_split_path(dev, small, dtype):
    c = small(dtype)
    m, x, v = c["m"], c["x"], c["v"]
    # the premise, without rows: one native call == the three of the split path
    split_plain = _split(m, x)
    d0 = float((c["plain"] - split_plain).abs().max())
    print(f"{dtype}: premise max |fused - split| without rows {d0:.3e}")
    assert torch.equal(c["plain"], split_plain)
    fused = m._c_forward(x, training=False, rows=v)
    split = _split(m, x, v)
    print(f"{dtype}: max |fused - split| with rows {float((fused - split).abs().max()):.3e}, "
          f"max |rows - plain| {float((fused - c['plain']).abs().max()):.3e}")
    assert torch.equal(fused, split)
    assert not torch.equal(fused, c["plain"])            # the rows arrived
    zero = m._c_forward(x, training=False, rows=torch.zeros_like(v))
    assert torch.equal(zero, c["plain"])
    with pytest.raises(RuntimeError, match="eval-mode"):
        m._c_forward(x, training=True, rows=v)
    with pytest.raises(RuntimeError, match="H/32"):
        m._c_forward(x, training=False, rows=v[:, :2].contiguous())
    assert torch.equal(m.eval_logits(x, bottleneck_rows=v), fused)
    assert torch.equal(m._c_forward(x, training=False), c["plain"])


# ------------------------------------------------------------------------------------------------ 3. per-call hygiene
def test_rowvec_request_is_one_shot_on_every_path(dev, small):
    """The rows are an option of ONE call: a forward that was refused with them, or ran with them, leaves nothing for the next."""
    import ctypes as C
    from flair_amd import _lib as L
    c = small("f32")
    m, x, v, plain = c["m"], c["x"], c["v"], c["plain"]
    l = L.lib()
    h = m._hh(False)
    B, _, H, W = x.shape
    # rows, then a plain forward that reuses the constants of the one before it
    with _env("FLAIR_EVAL_GRAPH", "0"):
        m._eval.key = None
        with_rows = m._c_forward(x, training=False, rows=v)
        key = m._eval.key
        again = m._c_forward(x, training=False)
        assert m._eval.key == key                          # (same key: this forward ran with reuse_constants = 1)
    assert torch.equal(again, plain) and not torch.equal(with_rows, plain)
    # rows on a refused shape, then a plain forward
    ws = m._workspace(B, H, W, False)
    out = torch.empty_like(plain)
    rows = L.UnetFwdOpts(rows_f32=L.ptr(v))
    with torch.cuda.device(dev):
        rc = l.flair_unet_forward(h, L.ptr(m._flat_p), L.ptr(m._flat_b), L.ptr(x), L.ptr(out), B, 48, W, 0, L.ptr(ws), ws.numel(), L.stream(),
                                  C.byref(rows))
        assert rc == -10
        L.check(l.flair_unet_forward(h, L.ptr(m._flat_p), L.ptr(m._flat_b), L.ptr(x), L.ptr(out), B, H, W, 0, L.ptr(ws), ws.numel(),
                                     L.stream(), None), "forward")
    assert torch.equal(out, plain)
    # rows alone on a training forward: refused with its code, nothing runs and nothing is kept
    m._eval.key = None
    wst = m._workspace(B, H, W, True)
    buffers = m._flat_b.clone()
    with torch.cuda.device(dev):
        rc = l.flair_unet_forward(m._h, L.ptr(m._flat_p), L.ptr(m._flat_b), L.ptr(x), L.ptr(out), B, H, W, 1, L.ptr(wst), wst.numel(),
                                  L.stream(), C.byref(rows))
        assert rc == -16 and b"rows_f32" in l.flair_strerror(rc)
        assert torch.equal(m._flat_b, buffers)             # nothing ran
        L.check(l.flair_unet_forward(m._h, L.ptr(m._flat_p), L.ptr(m._flat_b), L.ptr(x), L.ptr(out), B, H, W, 0, L.ptr(wst), wst.numel(),
                                     L.stream(), None), "forward")
    assert torch.equal(out, plain)
    # a malformed struct (a gradient pointer without rows) and a null handle: -1, nothing runs
    out.fill_(3.0)
    bad = L.UnetFwdOpts(drows_f32=L.ptr(v))
    with torch.cuda.device(dev):
        assert l.flair_unet_forward(h, L.ptr(m._flat_p), L.ptr(m._flat_b), L.ptr(x), L.ptr(out), B, H, W, 0, L.ptr(ws), ws.numel(),
                                    L.stream(), C.byref(bad)) == -1
        assert l.flair_unet_forward(None, L.ptr(m._flat_p), L.ptr(m._flat_b), L.ptr(x), L.ptr(out), B, H, W, 0, L.ptr(ws), ws.numel(),
                                    L.stream(), C.byref(rows)) == -1
    assert torch.equal(out, torch.full_like(out, 3.0)) and torch.equal(m._flat_b, buffers)
    assert torch.equal(m._c_forward(x, training=False), plain)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_forward_options_are_read_not_consumed(dev, dtype):
    """One struct (preds + maxprob + rows) serves two consecutive forwards alike, and a forward with opts = NULL on the same handle
    does none of it: the struct is an argument, the handle keeps nothing of it."""
    import ctypes as C
    from flair_amd import _lib as L
    _, m = _pair(5, 13, 23, dev, dtype)
    _, untouched = _pair(5, 13, 23, dev, dtype)
    m, untouched = m.eval(), untouched.eval()
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 5, 64, 64, generator=g).to(dev)
    v = torch.randn(1, 2, generator=g).to(dev)
    m._c_forward(x, training=False)   # flat parameters, eval handle and workspace exist
    l, h, ws = L.lib(), m._hh(False), m._workspace(1, 64, 64, False)
    preds = torch.empty(1, 64, 64, dtype=torch.uint8, device=dev)
    prob = torch.empty(1, 64, 64, dtype=torch.float32, device=dev)
    opts = L.UnetFwdOpts(preds_u8=L.ptr(preds), maxprob_f32=L.ptr(prob), rows_f32=L.ptr(v))

    def fwd(logits, opts):
        preds.fill_(99)
        prob.fill_(-1.0)
        with torch.cuda.device(dev):
            L.check(l.flair_unet_forward(h, L.ptr(m._flat_p), L.ptr(m._flat_b), L.ptr(x), L.ptr(logits), 1, 64, 64, 0, L.ptr(ws), ws.numel(),
                                         L.stream(), None if opts is None else C.byref(opts)), "forward")
        return preds.clone(), prob.clone()

    first, second = fwd(None, opts), fwd(None, opts)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    assert int((first[0] >= 13).sum()) == 0 and bool(((first[1] > 0) & (first[1] <= 1)).all())      # written, every pixel
    want = untouched.predict_classes(x, want_prob=True, bottleneck_rows=v)
    assert torch.equal(first[0], want[0]) and torch.equal(first[1], want[1])                        # ... with the rows
    logits = torch.empty(1, 13, 64, 64, dtype=torch.float32, device=dev)
    for out in (None, logits):     # (without fp32 logits a forward that still held the pointers would use them)
        after = fwd(out, None)
        assert int((after[0] != 99).sum()) == 0 and bool((after[1] == -1.0).all())
    assert torch.equal(logits, untouched._c_forward(x, training=False))                             # ... and no rows


# ------------------------------------------------------------------------------------------------ 4. graph replay
def test_predict_with_rows_replays_a_graph_that_takes_fresh_rows(dev):
    _, m = _pair(5, 13, 19, dev)
    m = m.eval()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 5, 512, 512, generator=g).to(dev)
    vs = [torch.randn(1, 16, generator=g).to(dev) for _ in range(5)]
    with _env("FLAIR_EVAL_GRAPH", "0"):
        want = [m.predict_classes(x, bottleneck_rows=v).clone() for v in vs]
        assert len(m._eval.graphs) == 0
    assert not torch.equal(want[0], want[1])
    m._eval.key = None
    assert os.environ.get("FLAIR_EVAL_GRAPH") is None
    for i, (v, w) in enumerate(zip(vs, want)):
        got = m.predict_classes(x, bottleneck_rows=v)
        assert torch.equal(got, w), (i, int((got != w).sum()))
        assert (len(m._eval.graphs) > 0) == (i >= 2)       # calls 3 to 5 replay
    assert list(m._eval.graphs) == [(False, True, False, True)]
    # the plain key has a graph of its own and never sees the rows
    plain = [m.predict_classes(x).clone() for _ in range(3)]
    assert torch.equal(plain[0], plain[2]) and not torch.equal(plain[2], want[4]) and len(m._eval.graphs) == 2


# ------------------------------------------------------------------------------------------------ 5. head epilogue
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_predict_classes_with_rows_equals_argmax_of_the_fused_logits(dev, small, dtype):
    """The probability is held to the 1e-6 the head epilogue's own operator test applies (against the fp64 softmax of the logits)."""
    from flair_amd import ops
    c = small(dtype)
    m, x, v = c["m"], c["x"], c["v"]
    logits = m._c_forward(x, training=False, rows=v)
    preds, prob = m.predict_classes(x, want_prob=True, bottleneck_rows=v)
    ref = ops.softmax_argmax(logits, want="u8")
    assert preds.dtype == torch.uint8 and torch.equal(preds, ref), int((preds != ref).sum())
    p64 = torch.softmax(logits.double().cpu(), dim=1).max(dim=1).values
    err = float((prob.cpu().double() - p64).abs().max())
    print(f"{dtype}: max |prob - softmax_fp64| {err:.3e}")
    assert err <= 1e-6
    assert torch.equal(m.predict_classes(x, bottleneck_rows=v), preds)


# ------------------------------------------------------------------------------------------------ 6. - 8. config 4 at 512 x 512
@pytest.fixture(scope="module")
def config4(dev, golden_dir):
    """The model of test_golden_metadata_path_fp32 (FLAIR_ModelFactory, 19 classes, metadata, fp32, seed 2023), its oracle twin, the
    golden tile and metadata; a second tile / metadata row for batches of two.  Shared, never modified."""
    import flair_amd
    from oracle import unet_resnet34 as om
    gm = np.load(os.path.join(golden_dir, "metadata_c19_512.npz"))
    state = torch.random.get_rng_state()
    torch.manual_seed(2023)
    try:
        enc_ref = flair_amd.MetadataMLP()
        ref = om.create_model("unet", "resnet34", in_channels=5, classes=19)
    finally:
        torch.random.set_rng_state(state)
    model = flair_amd.FLAIR_ModelFactory(_config(5, CLASSES19, use_metadata=True), compute_dtype="f32")
    model.enc.load_state_dict(enc_ref.state_dict())
    model.seg_model.load_state_dict(ref.state_dict())
    model = model.to(dev).eval()
    g = torch.Generator().manual_seed(int(gm["tile_seed"]))
    tile = torch.randn(1, 5, 512, 512, generator=g)
    mtd = torch.from_numpy(gm["mtd"])
    g2 = torch.Generator().manual_seed(77)
    tile2 = torch.randn(1, 5, 512, 512, generator=g2)
    mtd2 = torch.rand(1, 45, generator=g2)
    yield dict(gm=gm, model=model, ref=ref.eval(), enc_ref=enc_ref.eval(), tile=tile, mtd=mtd,
               img2=torch.cat([tile, tile2]), mtd2=torch.cat([mtd.float(), mtd2]))
    torch.cuda.empty_cache()


def test_golden_metadata_fused_path_fp32(dev, config4):
    gm, model = config4["gm"], config4["model"]
    tile, mtd = config4["tile"].to(dev), config4["mtd"].to(dev)
    assert os.environ.get("FLAIR_META_FUSE") is None
    with torch.no_grad():
        lg_d = model(tile, mtd)
        with _env("FLAIR_META_FUSE", "0"):
            lg_split = model(tile, mtd)
            # the premise of the bit comparison below: without rows the two paths agree bit for bit
            sm = model.seg_model
            assert torch.equal(sm._c_forward(tile, training=False), _split(sm, tile))
    lg = lg_d.cpu()
    scale = np.abs(gm["logits_crop"]).max()
    assert np.abs(lg[0, :, 100:132, 300:332].numpy() - gm["logits_crop"]).max() < 1e-3 * max(1.0, scale)
    assert np.abs(lg.double().mean(dim=(0, 2, 3)).numpy() - gm["logits_mean"]).max() < 1e-3
    print("max |fused - split|", float((lg_d - lg_split).abs().max()))
    assert torch.equal(lg_d, lg_split)
    with pytest.raises(RuntimeError, match="512x512"):
        model(tile[:, :, :256, :256].contiguous(), mtd)


def test_seg_trainer_validate_and_predict_with_metadata(dev, config4):
    """B = 2, 512 x 512, the 19 YAML class weights, fp32: against ref.eval() + metadata add + oracle.seg_step.step_torch on the CPU
    at the bar of test_validate_step_against_the_oracle (loss within 2e-3, predictions equal where the oracle's top-2 logit gap
    exceeds 2e-3)."""
    import flair_amd
    from oracle import seg_step
    C = 19
    model, ref, enc_ref = config4["model"], config4["ref"], config4["enc_ref"]
    img, mtd = config4["img2"], config4["mtd2"]
    g = torch.Generator().manual_seed(3)
    lab = torch.randint(0, C, (2, 512, 512), generator=g)
    onehot = torch.nn.functional.one_hot(lab, C).permute(0, 3, 1, 2).contiguous().float()
    w = torch.tensor([float(v[0]) for v in CLASSES19.values()])
    with torch.no_grad():
        feats = ref.encoder(img)
        x_enc = enc_ref(mtd)
        feats[-1] = feats[-1] + x_enc.unsqueeze(1).unsqueeze(-1).repeat(1, 512, 1, 16)   # model.py:59-60
        logits = ref.segmentation_head(ref.decoder(*feats))
        loss_ref, preds_ref, _ = seg_step.step_torch(logits, onehot, w)
    sm = model.seg_model
    tr = flair_amd.SegTrainer(sm, lr=0.0, class_weight=w, metadata_encoder=model.enc)
    before = (sm.flat_parameters().clone(), sm.flat_buffers().clone(), sm._flat_n.clone())
    loss = tr.validate_step(img.to(dev), onehot.to(dev), mtd.to(dev)).item()
    print("oracle:", loss_ref.item(), "hip:", loss)
    assert abs(loss - loss_ref.item()) <= 2e-3
    top2 = logits.topk(2, dim=1).values
    sure = (top2[:, 0] - top2[:, 1]) > 2e-3
    val_preds = tr._val_preds.clone()
    preds = val_preds.cpu().to(torch.int64)
    assert sure.float().mean() > 0.9
    assert torch.equal(preds[sure], preds_ref.view(2, 512, 512)[sure])
    # the metadata matters: without it the loss differs
    tr_plain = flair_amd.SegTrainer(sm, lr=0.0, class_weight=w)
    assert tr_plain.validate_step(img.to(dev), onehot.to(dev)).item() != loss
    # confusion matrix increment = host bincount of the predictions
    cm_ref = seg_step.confusion_matrix_np(lab.numpy(), val_preds.cpu().numpy(), C)
    assert np.array_equal(tr.val_confmat.cpu().numpy(), cm_ref) and cm_ref.sum() == lab.numel()
    assert torch.equal(tr.predict(img.to(dev), mtd.to(dev)), val_preds)
    assert all(torch.equal(u, v) for u, v in zip(before, (sm.flat_parameters(), sm.flat_buffers(), sm._flat_n)))
    with pytest.raises(ValueError, match="metadata_encoder"):
        tr_plain.validate_step(img.to(dev), onehot.to(dev), mtd.to(dev))
    with pytest.raises(ValueError, match="metadata_encoder"):
        tr_plain.predict(img.to(dev), mtd.to(dev))


def test_validation_with_metadata_leaves_training_alone(dev):
    """As test_validation_leaves_training_alone: a validate_step with metadata between two training steps changes no parameter, buffer
    or batch counter and the second step computes what it computes without it."""
    import flair_amd
    C = 13
    _, a = _pair(5, C, 5, dev)
    _, b = _pair(5, C, 5, dev)
    enc = flair_amd.MetadataMLP().to(dev).train()      # (its mode does not matter: eval-mode steps encode without dropout)
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(2, 5, 64, 64, generator=g).to(dev) for _ in range(2)]
    labs = [torch.randint(0, C, (2, 64, 64), generator=g).to(torch.uint8).to(dev) for _ in range(2)]
    xv = torch.randn(1, 5, 512, 512, generator=g).to(dev)
    labv = torch.randint(0, C, (1, 512, 512), generator=g).to(torch.uint8).to(dev)
    mtd = torch.rand(1, 45, generator=g).to(dev)
    w = torch.linspace(0.5, 2, C)
    ta = flair_amd.SegTrainer(a.train(), lr=0.02, class_weight=w, metadata_encoder=enc)
    tb = flair_amd.SegTrainer(b.train(), lr=0.02, class_weight=w)
    la0 = ta.train_step(xs[0], labs[0]).item()
    before = (a.flat_parameters().clone(), a.flat_buffers().clone(), a._flat_n.clone())
    l1 = ta.validate_step(xv, labv, mtd).clone()
    l2 = ta.validate_step(xv, labv, mtd)
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))   # no dropout, although the encoder is in training mode
    assert all(torch.equal(u, v) for u, v in zip(before, (a.flat_parameters(), a.flat_buffers(), a._flat_n)))
    la1 = ta.train_step(xs[1], labs[1]).item()
    lb0 = tb.train_step(xs[0], labs[0]).item()
    lb1 = tb.train_step(xs[1], labs[1]).item()
    assert (la0, la1) == (lb0, lb1)
    assert torch.equal(a.flat_parameters(), b.flat_parameters()) and torch.equal(a.flat_buffers(), b.flat_buffers())
    assert torch.equal(a._flat_n, b._flat_n)


@pytest.mark.parametrize("use_metadata", [True, False], ids=["metadata", "plain"])
def test_predict_step_takes_the_argmax_from_the_head_epilogue(dev, config4, use_metadata):
    """batch['preds'] int64 and equal to what predict_step computed before it had the fast path: softmax_argmax over the logits of
    forward() (with metadata: of the split path)."""
    import flair_amd
    from flair_amd import ops
    if use_metadata:
        model = config4["model"]
    else:
        model = flair_amd.FLAIR_ModelFactory(_config(5, CLASSES19), compute_dtype="f32")
        model.seg_model.load_state_dict(config4["ref"].state_dict())
        model = model.to(dev).eval()
    task = flair_amd.segmentation_task_predict(model, num_classes=19, use_metadata=use_metadata)
    img, mtd = config4["tile"].to(dev), config4["mtd"].to(dev)
    with torch.no_grad(), _env("FLAIR_META_FUSE", "0"):
        logits = model(img, mtd) if use_metadata else model(img)
        old = ops.softmax_argmax(logits.detach().float().contiguous(), want="i64")
    batch = {"img": img, "id": ["x"]}
    if use_metadata:
        batch["mtd"] = mtd
    out = task.predict_step(batch, 0)
    assert out is batch and set(out) == set(batch)
    assert out["preds"].dtype == torch.int64 and out["preds"].shape == (1, 512, 512)
    assert torch.equal(out["preds"], old), int((out["preds"] != old).sum())
    # FLAIR_ModelFactory.predict_classes itself, probability included
    pr, pb = model.predict_classes(img, mtd if use_metadata else None, want_prob=True)
    assert pr.dtype == torch.uint8 and torch.equal(pr.to(torch.int64), old) and pb.dtype == torch.float32
    if use_metadata:
        with pytest.raises(ValueError, match="metadata"):
            model.predict_classes(img)
    # a training-mode model keeps the present code
    if not use_metadata:   # (this model is the test's own: the training-mode forward moves its running statistics)
        model.train()
        with torch.no_grad():
            out_t = task.predict_step({"img": img, "id": ["x"]}, 0)
        model.eval()
        assert out_t["preds"].dtype == torch.int64 and out_t["preds"].shape == (1, 512, 512)
        assert not torch.equal(out_t["preds"], old)        # batch statistics: another forward altogether
