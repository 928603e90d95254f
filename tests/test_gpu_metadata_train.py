"""Metadata in the native training step (BASELINE config 4): the bottleneck row add of model.py:59-60 inside ONE training forward
(rows_f32 + drows_f32 of flair_unet_fwd_opts_t: a second tensor for the decoder, the encoder's output stays as the ReLU mask source of its unit), the
gradient of the rows out of the native backward (flair_rowvec_grad_nhwc), and SegTrainer.train_step(img, labels, mtd), which also
trains the MetadataMLP.

Sections: 1 the two operators (exact integer sums, the any-order rounding bound, refusals), 2 the executor on the 2x5x160x128 batch
of test_train_step_matches_oracle_elementwise_fp32 (zero rows are invisible bit for bit; large positive rows, which an in-place add
would turn into wrong ReLU masks, against the CPU fp32 and fp64 oracles; per-call hygiene; workspace), 3 SegTrainer at 512 x 512,
4 two ranks on one GPU."""
import copy
import ctypes as C
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

import metadata_train_cases as tc
from parity_helpers import assert_as_good_as_cpu_fp32

pytestmark = pytest.mark.gpu

CLASSES19 = {1: [1, 'building'], 2: [1, 'pervious surface'], 3: [1, 'impervious surface'], 4: [1, 'bare soil'],
             5: [1, 'water'], 6: [1, 'coniferous'], 7: [1, 'deciduous'], 8: [1, 'brushwood'], 9: [1, 'vineyard'],
             10: [1, 'herbaceous vegetation'], 11: [1, 'agricultural land'], 12: [1, 'plowed land'],
             13: [1, 'swimming_pool'], 14: [1, 'snow'], 15: [0, 'clear cut'], 16: [0, 'mixed'], 17: [0, 'ligneous'],
             18: [1, 'greenhouse'], 19: [0, 'other']}
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
SMALL = (2, 5, 160, 128)    # bottleneck 5 rows x 4 columns


def _pair(in_ch, classes, seed, dev, dtype="f32"):
    import flair_amd
    from oracle import unet_resnet34 as om
    ref = om.seeded_model(in_ch, classes, seed)
    hip = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=in_ch, classes=classes, compute_dtype=dtype)
    hip.load_state_dict(ref.state_dict(), strict=True)
    return ref, hip.to(dev)


def _seeded_mlp(seed):
    import flair_amd
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        return flair_amd.MetadataMLP()
    finally:
        torch.random.set_rng_state(state)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ------------------------------------------------------------------------------------------------ 1. operators
def _add_to(x, v, y):
    from flair_amd import _lib as L
    N, H, W, C = x.shape
    return L.lib().flair_add_rowvec_nhwc_to(L.dtype_code(x.dtype), L.ptr(x), L.ptr(v), L.ptr(y), N, H, W, C, L.stream())


def _row_grad(dx, dv):
    from flair_amd import _lib as L
    N, H, W, C = dx.shape
    return L.lib().flair_rowvec_grad_nhwc(L.dtype_code(dx.dtype), L.ptr(dx), L.ptr(dv), N, H, W, C, L.stream())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", tc.ADD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_add_rowvec_nhwc_to_equals_clone_plus_the_in_place_add(dev, shape, dtype):
    from flair_amd import _lib as L
    x, v, want = tc.add_case(shape, DTYPES[dtype])
    xd, vd = x.to(dev), v.to(dev)
    inplace = xd.clone()
    N, H, W, C = shape
    assert L.lib().flair_add_rowvec_nhwc(L.dtype_code(xd.dtype), L.ptr(inplace), L.ptr(vd), N, H, W, C, L.stream()) == 0
    y = torch.full_like(xd, 7.0)
    assert _add_to(xd, vd, y) == 0
    assert torch.equal(_bits(y), _bits(inplace)) and torch.equal(_bits(y.cpu()), _bits(want))
    assert torch.equal(_bits(xd.cpu()), _bits(x))                # the source is untouched
    assert _add_to(xd, vd, xd) == 0                              # x == y: the in-place function
    assert torch.equal(_bits(xd), _bits(inplace))


def test_add_rowvec_nhwc_to_refuses_what_the_in_place_add_refuses(dev):
    from flair_amd import _lib as L
    l = L.lib()
    x = torch.zeros(1, 2, 2, 32, device=dev)
    y = torch.full_like(x, 3.0)
    v = torch.ones(1, 2, device=dev)
    before = y.clone()
    for C in (4, 12, 20):
        assert l.flair_add_rowvec_nhwc_to(0, L.ptr(x), L.ptr(v), L.ptr(y), 1, 2, 2, C, L.stream()) == -2
    assert l.flair_add_rowvec_nhwc_to(0, x.data_ptr() + 4, L.ptr(v), L.ptr(y), 1, 2, 2, 8, L.stream()) == -2
    assert l.flair_add_rowvec_nhwc_to(0, L.ptr(x), L.ptr(v), y.data_ptr() + 4, 1, 2, 2, 8, L.stream()) == -2
    assert l.flair_add_rowvec_nhwc_to(2, L.ptr(x), L.ptr(v), L.ptr(y), 1, 2, 2, 8, L.stream()) == -2
    assert l.flair_add_rowvec_nhwc_to(0, None, L.ptr(v), L.ptr(y), 1, 2, 2, 8, L.stream()) == -1
    assert l.flair_add_rowvec_nhwc_to(0, L.ptr(x), None, L.ptr(y), 1, 2, 2, 8, L.stream()) == -1
    assert l.flair_add_rowvec_nhwc_to(0, L.ptr(x), L.ptr(v), None, 1, 2, 2, 8, L.stream()) == -1
    assert torch.equal(y, before)
    # the gradient's refusals, output untouched
    dv = torch.full((1, 2), 5.0, device=dev)
    for C in (4, 12, 20):
        assert l.flair_rowvec_grad_nhwc(0, L.ptr(x), L.ptr(dv), 1, 2, 2, C, L.stream()) == -2
    assert l.flair_rowvec_grad_nhwc(0, x.data_ptr() + 4, L.ptr(dv), 1, 2, 2, 8, L.stream()) == -2
    assert l.flair_rowvec_grad_nhwc(2, L.ptr(x), L.ptr(dv), 1, 2, 2, 8, L.stream()) == -2
    assert l.flair_rowvec_grad_nhwc(0, None, L.ptr(dv), 1, 2, 2, 8, L.stream()) == -1
    assert l.flair_rowvec_grad_nhwc(0, L.ptr(x), None, 1, 2, 2, 8, L.stream()) == -1
    assert torch.equal(dv, torch.full_like(dv, 5.0))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", tc.GRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rowvec_grad_nhwc_is_exact_on_integers(dev, shape, dtype):
    dx, want = tc.int_case(shape, DTYPES[dtype])
    dxd = dx.to(dev)
    dv = torch.full(shape[:2], float("nan"), device=dev)
    assert _row_grad(dxd, dv) == 0
    assert torch.equal(_bits(dv.cpu()), _bits(want)), (dv.cpu(), want)
    assert torch.equal(_bits(dxd.cpu()), _bits(dx))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", tc.GRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rowvec_grad_nhwc_random_inputs_within_the_any_order_bound_and_repeatable(dev, shape, dtype):
    dx, s64, bound = tc.normal_case(shape, DTYPES[dtype])
    dxd = dx.to(dev)
    dv1 = torch.full(shape[:2], float("nan"), device=dev)
    dv2 = torch.full(shape[:2], float("nan"), device=dev)
    assert _row_grad(dxd, dv1) == 0 and _row_grad(dxd, dv2) == 0
    err = (dv1.cpu().double() - s64).abs()
    print(f"{dtype} {shape}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3e}")
    assert bool((err <= bound).all()), (err, bound)
    assert torch.equal(_bits(dv1), _bits(dv2))


# ------------------------------------------------------------------------------------------------ 2. the executor, small
def _dlogits(logits, lab, C):
    """d mean-CE / d logits, elementwise (deterministic): (softmax - onehot) / pixels."""
    onehot = torch.nn.functional.one_hot(lab.long(), C).permute(0, 3, 1, 2).float()
    return ((torch.softmax(logits, dim=1) - onehot) / lab.numel()).contiguous()


def _hip_step(c, rows=None, drows=None):
    """One training forward + backward of the case's model from its initial buffers; returns logits, flat gradients, buffers, counters."""
    m = c["m"]
    m._flat_b.copy_(c["b0"]); m._flat_n.copy_(c["n0"])
    logits = m._c_forward(c["x"], training=True, train_rows=None if rows is None else (rows, drows))
    grads = m._c_backward(dlogits=_dlogits(logits, c["lab"], 13), grads=torch.zeros_like(m._flat_p))
    torch.cuda.synchronize()
    return dict(logits=logits, grads=grads, b=m._flat_b.clone(), n=m._flat_n.clone())


@pytest.fixture(scope="module")
def small(dev):
    """case(dtype) -> the model of test_train_step_matches_oracle_elementwise_fp32 (seed 123, 13 classes) in training mode, its batch,
    the initial buffers and the PLAIN training step from them; built once, the plain step never modified."""
    built = {}

    def case(dtype):
        if dtype not in built:
            ref, m = _pair(5, 13, 123, dev, dtype)
            m = m.train()
            g = torch.Generator().manual_seed(5)
            x = torch.randn(*SMALL, generator=g)
            lab = torch.randint(0, 13, (2, 160, 128), generator=g)
            m.flatten_()
            c = dict(m=m, ref=ref, x=x.to(dev), lab=lab.to(dev), x_cpu=x, lab_cpu=lab, b0=m._flat_b.clone(), n0=m._flat_n.clone())
            c["plain"] = _hip_step(c)
            built[dtype] = c
        return built[dtype]

    yield case
    built.clear()
    torch.cuda.empty_cache()


def _same_step(a, b):
    return {k: bool(torch.equal(_bits(a[k]) if a[k].is_floating_point() else a[k], _bits(b[k]) if b[k].is_floating_point() else b[k]))
            for k in ("logits", "grads", "b", "n")}


ALL_SAME = {"logits": True, "grads": True, "b": True, "n": True}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_zero_rows_are_invisible(dev, small, dtype):
    c = small(dtype)
    rows = torch.zeros(2, 5, device=dev)
    drows = torch.full((2, 5), float("nan"), device=dev)
    got = _hip_step(c, rows, drows)
    assert _same_step(got, c["plain"]) == ALL_SAME
    assert bool(torch.isfinite(drows).all()) and bool((drows != 0).all()), drows
    assert bool(torch.isfinite(got["grads"]).all()) and float(got["grads"].abs().max()) > 0


def _oracle(ref, x, lab, v):
    """model.py:57-62 on the CPU oracle in training mode with v a leaf: logits, parameter gradients, d loss / d v."""
    ref.train()
    ref.zero_grad()
    v = v.clone().requires_grad_(True)
    feats = ref.encoder(x)
    feats[-1] = feats[-1] + v[:, None, :, None]
    o = ref.segmentation_head(ref.decoder(*feats))
    nn.functional.cross_entropy(o, lab).backward()
    return o.detach(), {k: p.grad.detach().clone() for k, p in ref.named_parameters()}, v.grad.detach().clone()


def _tensor_errs(got, truth):
    return {k: tc.rel_max_err(got[k], truth[k]) for k in truth}


@pytest.mark.parametrize("kind", ["large_positive", "randn"])
def test_rows_step_matches_the_oracles_fp32(dev, small, kind):
    """large_positive: rows of 50.0, far above every bottleneck activation — added in place they would turn every zero of layer4's
    last ReLU output into 'ReLU on' for that unit's backward, and the encoder's gradients would be wrong throughout.  randn: ordinary
    rows, negative values included.  Logits within 1e-3 of the CPU fp32 and fp64 oracles; parameter gradients as good as CPU fp32's
    against fp64 (whole-model bounds 1.5 / 2.0 / 3.0); d rows by the same rule as a set of one tensor: relative max-norm error
    against fp64 <= 3.0 x CPU fp32's + 2e-2.

    Measured on the MI355X (profiles/metadata_train_parity.json), HIP / CPU-fp32 error ratios at median / 90th percentile / maximum:
    large_positive 1.03 / 1.10 / 1.00, randn 1.34 / 1.02 / 1.00; d rows 2.3e-2 against 1.7e-2 (1.33x) and 7.2e-3 against 6.1e-4
    (inside the additive 2e-2).  An executor built with the add in place fails both cases at the first bound: median gradient error
    0.26 (large_positive) and 0.45 (randn) against CPU fp32's 0.014 and 0.005."""
    from oracle import parity
    c = small("f32")
    m = c["m"]
    v = torch.full((2, 5), 50.0) if kind == "large_positive" else torch.randn(2, 5, generator=torch.Generator().manual_seed(21))
    drows = torch.full((2, 5), float("nan"), device=dev)
    got = _hip_step(c, v.to(dev), drows)
    ref = c["ref"]
    ref64 = copy.deepcopy(ref).double()
    o32, g32, dv32 = _oracle(ref, c["x_cpu"], c["lab_cpu"], v)
    o64, g64, dv64 = _oracle(ref64, c["x_cpu"].double(), c["lab_cpu"], v.double())
    lg = got["logits"].cpu()
    d32, d64 = float((lg - o32).abs().max()), float((lg.double() - o64).abs().max())
    print(f"{kind}: max |logits - cpu fp32| {d32:.3e}, - fp64 {d64:.3e}")
    assert d32 < 1e-3 and d64 < 1e-3
    assert not torch.equal(got["logits"], c["plain"]["logits"])          # the rows arrived
    hip_g = dict(zip(m._param_names, [t.cpu() for t in m._grad_views(got["grads"])]))
    assert sorted(hip_g) == sorted(g64)
    suffix = "" if kind == "large_positive" else "_randn"
    assert_as_good_as_cpu_fp32(_tensor_errs(hip_g, g64), _tensor_errs(g32, g64), "grad_vs_fp64_rows_train_2x5x160x128" + suffix)
    e_hip, e_cpu = tc.rel_max_err(drows, dv64), tc.rel_max_err(dv32, dv64)
    entry = {"test": "drows_vs_fp64_rows_train_2x5x160x128" + suffix, "err_hip": e_hip, "err_cpu_fp32": e_cpu,
             "ratio": e_hip / max(e_cpu, 1e-30)}
    parity.record(entry)
    print(entry)
    assert e_hip <= 3.0 * e_cpu + 2e-2, entry


def test_train_request_hygiene(dev, small):
    from flair_amd import _lib as L
    c = small("f32")
    m, x, plain = c["m"], c["x"], c["plain"]
    l = L.lib()
    B, _, H, W = x.shape
    v = torch.full((2, 5), 2.0, device=dev)
    drows = torch.full((2, 5), 7.0, device=dev)
    sentinel = drows.clone()
    # the Python argument
    with pytest.raises(RuntimeError, match="training-mode"):
        m._c_forward(x, training=False, train_rows=(v, drows))
    with pytest.raises(RuntimeError, match="exclude"):
        m._c_forward(x, training=True, rows=v, train_rows=(v, drows))
    with pytest.raises(RuntimeError, match="eval-mode"):
        m._c_forward(x, training=True, rows=v)
    with pytest.raises(RuntimeError, match="H/32"):
        m._c_forward(x, training=True, train_rows=(v[:, :4].contiguous(), drows))
    # the request meets an eval-mode forward: -17, nothing runs; a plain eval forward afterwards is the plain one
    m._flat_b.copy_(c["b0"]); m._flat_n.copy_(c["n0"])
    m._eval.key = None
    eval_plain = m._c_forward(x, training=False).clone()
    h = m._hh(False)
    ws = m._workspace(B, H, W, False)
    out = torch.full_like(eval_plain, 3.0)
    buffers = m._flat_b.clone()
    both = L.UnetFwdOpts(rows_f32=L.ptr(v), drows_f32=L.ptr(drows))

    def fwd(handle, H_, training, arena, opts):
        return l.flair_unet_forward(handle, L.ptr(m._flat_p), L.ptr(m._flat_b), L.ptr(x), L.ptr(out), B, H_, W, training, L.ptr(arena),
                                    arena.numel(), L.stream(), None if opts is None else C.byref(opts))

    with torch.cuda.device(dev):
        rc = fwd(h, H, 0, ws, both)
        assert rc == -17 and b"drows_f32" in l.flair_strerror(rc)
        torch.cuda.synchronize()
        assert torch.equal(out, torch.full_like(out, 3.0)) and torch.equal(m._flat_b, buffers) and torch.equal(drows, sentinel)
        # malformed structs: a gradient pointer without rows, in either mode, and a null handle
        wst = m._workspace(B, H, W, True)
        assert fwd(h, H, 0, ws, L.UnetFwdOpts(drows_f32=L.ptr(drows))) == -1
        assert fwd(m._h, H, 1, wst, L.UnetFwdOpts(drows_f32=L.ptr(drows))) == -1
        assert fwd(None, H, 1, wst, both) == -1
        torch.cuda.synchronize()
        assert torch.equal(out, torch.full_like(out, 3.0)) and torch.equal(m._flat_b, buffers) and torch.equal(drows, sentinel)
        L.check(fwd(h, H, 0, ws, None), "forward")
    assert torch.equal(out, eval_plain)
    m._eval.key = None
    with torch.cuda.device(dev):
        # rows without a gradient pointer still refuse a training forward with their own code
        rc = fwd(m._h, H, 1, wst, L.UnetFwdOpts(rows_f32=L.ptr(v)))
        assert rc == -16
        # both on a refused shape, then a plain training forward + backward: the plain step, d rows not written
        assert fwd(m._h, 48, 1, wst, both) == -10
    assert torch.equal(m._flat_b, buffers)
    assert _same_step(_hip_step(c), plain) == ALL_SAME
    assert torch.equal(drows, sentinel)
    # two consecutive steps, the first with rows, the second without: the second is the plain one
    first = _hip_step(c, v, drows)
    assert not torch.equal(drows, sentinel) and not torch.equal(first["logits"], plain["logits"])
    kept = drows.clone()
    assert _same_step(_hip_step(c), plain) == ALL_SAME
    assert torch.equal(drows, kept)


def test_bf16_rows_step_is_bit_reproducible(dev, small):
    c = small("bf16")
    v = torch.randn(2, 5, generator=torch.Generator().manual_seed(3)).to(dev)
    runs = []
    for _ in range(2):
        drows = torch.full((2, 5), float("nan"), device=dev)
        got = _hip_step(c, v, drows)
        got["drows"] = drows
        runs.append(got)
    assert _same_step(runs[0], runs[1]) == ALL_SAME
    assert torch.equal(_bits(runs[0]["drows"]), _bits(runs[1]["drows"])) and bool(torch.isfinite(runs[0]["drows"]).all())
    assert not torch.equal(runs[0]["logits"], c["plain"]["logits"])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_rows_step_fits_the_reported_workspace(dev, small, dtype):
    """The arena is sized by a dry run of the split sequence, which holds five re-imported feature tensors the fused forward never
    allocates: the extra bottleneck tensor of a rows step fits, flair_unet_workspace_bytes is what it was (pinned for this shape
    in test_metadata_train_cases_cpu.py) and a rows step in a workspace of exactly that size returns 0."""
    from flair_amd import _lib as L
    c = small(dtype)
    m = c["m"]
    B, _, H, W = c["x"].shape
    need = L.lib().flair_unet_workspace_bytes(m._h, B, H, W, 1)
    print(f"{dtype}: flair_unet_workspace_bytes {need}, pinned {tc.WORKSPACE_2x160x128[dtype][0]}")
    assert m._workspace(B, H, W, True).numel() == need
    drows = torch.full((2, 5), float("nan"), device=dev)
    got = _hip_step(c, torch.ones(2, 5, device=dev), drows)        # (L.check raises on -100, workspace too small)
    assert m._live.ws.numel() == need and bool(torch.isfinite(drows).all()) and bool(torch.isfinite(got["grads"]).all())


# ------------------------------------------------------------------------------------------------ 3. SegTrainer, 512 x 512
def _yaml_weights():
    return torch.tensor([float(v[0]) for v in CLASSES19.values()])


def _batch512(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 5, 512, 512, generator=g)
    mtd = torch.rand(B, 45, generator=g)
    lab = torch.randint(0, C, (B, 512, 512), generator=g)
    return x, mtd, lab


def _mlp_equal(a, b):
    return all(torch.equal(_bits(p.detach()), _bits(q.detach())) for p, q in zip(a.parameters(), b.parameters()))


def _by_hand(model, enc, tr, img, lab, mtd, masks, lr):
    """What train_step(img, lab, mtd, mtd_masks=masks) is documented to do, call by call (tr lends its head buffers)."""
    from flair_amd import _lib as L
    from flair_amd import ops
    l = L.lib()
    B, _, H, W = img.shape
    ld = tr._buffers(B, H, W)
    for p in enc.parameters():
        p.grad = None
    rows = enc(mtd, masks=masks)
    drows = torch.empty(B, 16, device=img.device)
    model._c_forward(img, training=True, want_logits=False, train_rows=(rows.detach(), drows))
    L.check(l.flair_ce_head_nhwc(l.flair_unet_logits_nhwc(model._h), model._dt, ld, L.ptr(lab), ops._LABEL_KIND[lab.dtype],
                                 L.ptr(tr.class_weight), B, model.classes, H, W, L.ptr(tr.loss), L.ptr(tr._dl), L.ptr(tr._preds), None,
                                 L.ptr(tr.confmat), L.ptr(tr._ce_ws), L.stream()), "ce_head_nhwc")
    model._c_backward(dlogits_nhwc=tr._dl, grads=tr.grads)
    rows.backward(drows)
    for p in enc.parameters():
        ops.sgd_step_(p.data, p.grad, lr)
        p.grad = None
    ops.sgd_step_(model._flat_p, tr.grads, lr)
    model._eval.note_native_write()
    return tr.loss.clone()


def test_train_step_with_metadata_is_the_documented_sequence_bit_for_bit(dev):
    import flair_amd
    C, lr = 13, 0.02
    _, a = _pair(5, C, 5, dev)
    _, b = _pair(5, C, 5, dev)
    enc_a, enc_b = _seeded_mlp(9).to(dev).train(), _seeded_mlp(9).to(dev).train()
    start = copy.deepcopy(enc_a)
    x, mtd, lab = _batch512(2, C, 4)
    x, mtd, lab = x.to(dev), mtd.to(dev), lab.to(torch.uint8).to(dev)
    g = torch.Generator().manual_seed(6)
    masks = [(torch.bernoulli(torch.full((2, n), 0.6), generator=g) / 0.6).to(dev) for n in (64, 32, 16)]
    w = torch.linspace(0.5, 2, C)
    ta = flair_amd.SegTrainer(a.train(), lr=lr, class_weight=w, metadata_encoder=enc_a)
    tb = flair_amd.SegTrainer(b.train(), lr=lr, class_weight=w)
    for step in range(2):     # the second step shows that no gradient of the first is left to accumulate
        la = ta.train_step(x, lab, mtd, mtd_masks=masks).clone()
        assert all(p.grad is None for p in enc_a.parameters())
        lb = _by_hand(b, enc_b, tb, x, lab, mtd, masks, lr)
        assert torch.equal(_bits(la), _bits(lb)), (step, float(la), float(lb))
        assert torch.equal(_bits(a.flat_parameters()), _bits(b.flat_parameters())), step
        assert torch.equal(_bits(a.flat_buffers()), _bits(b.flat_buffers())) and torch.equal(a._flat_n, b._flat_n)
        assert _mlp_equal(enc_a, enc_b), step
    assert not _mlp_equal(enc_a, start)                      # and the MLP did move
    assert enc_a.training                                      # the trainer does not switch the encoder's mode
    assert tuple(ta.mlp_grads.shape) == (sum(p.numel() for p in enc_a.parameters()),)


def test_plain_metadata_step_updates_two_flat_buffers_in_two_launches(dev):
    """(the bits are pinned by the test above)"""
    import flair_amd
    import launch_helpers as LH
    from flair_amd import flat
    C = 13
    _, m = _pair(5, C, 5, dev)
    enc = _seeded_mlp(9).to(dev).train()
    x, mtd, lab = _batch512(1, C, 14)
    x, mtd, lab = x.to(dev), mtd.to(dev), lab.to(torch.uint8).to(dev)
    tr = flair_amd.SegTrainer(m.train(), lr=0.02, metadata_encoder=enc)
    _, ran = LH.profiled(lambda: tr.train_step(x, lab, mtd), keep=("sgd", "optim_"), slots=2048)
    assert ran == {"optim_sgd": 2}, ran                      # the U-Net's buffer and the MLP's: not one launch per MLP tensor
    ps = [p for p in enc.parameters() if p.requires_grad]
    offs = [sum(p.numel() for p in ps[:i]) for i in range(len(ps))]
    assert len(ps) == 6 and tr._mlp_opt.flat.numel() == sum(p.numel() for p in ps)
    assert flat.aliased(tr._mlp_opt.flat, zip(ps, offs))
    assert tr.optimizer is None


def test_auto_masks_follow_the_encoders_mode_and_torchs_generator(dev):
    import flair_amd
    C = 13
    x, mtd, lab = _batch512(1, C, 14)
    x, mtd, lab = x.to(dev), mtd.to(dev), lab.to(torch.uint8).to(dev)
    res = []
    for mode in ("train", "train", "eval"):
        _, m = _pair(5, C, 5, dev)
        enc = _seeded_mlp(9).to(dev)
        enc = enc.train() if mode == "train" else enc.eval()
        tr = flair_amd.SegTrainer(m.train(), lr=0.02, metadata_encoder=enc)
        torch.manual_seed(11)
        loss = tr.train_step(x, lab, mtd).clone()
        res.append((loss, m.flat_parameters().detach().clone(), [p.detach().clone() for p in enc.parameters()]))
        assert enc.training == (mode == "train")
    same = lambda u, v: (torch.equal(_bits(u[0]), _bits(v[0])) and torch.equal(_bits(u[1]), _bits(v[1]))
                         and all(torch.equal(_bits(p), _bits(q)) for p, q in zip(u[2], v[2])))
    assert same(res[0], res[1])
    assert not torch.equal(res[0][0], res[2][0]) and not torch.equal(res[0][1], res[2][1])


def test_train_step_with_metadata_matches_the_oracle_fp32(dev):
    """B = 1, dropout off, 19 classes with the YAML weights — the batch and construction of test_split_path_training_matches_fused.
    CPU fp32 and fp64 oracles of model.py:57-62 with cross_entropy(weight=); U-Net and MLP gradients (read with lr = 0) as good as
    CPU fp32's against fp64 at that test's bounds 2.0 / 2.5 / 3.0; loss within 2e-4 relative."""
    import flair_amd
    from oracle import unet_resnet34 as om
    C = 19
    ref = om.seeded_model(5, C, 77)
    hip = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=C, compute_dtype="f32")
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip = hip.to(dev).train()
    enc_cpu = _seeded_mlp(78).eval()                           # dropout off for parity (quirk Q5)
    enc = copy.deepcopy(enc_cpu).to(dev).eval()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(1, 5, 512, 512, generator=g)
    mtd = torch.rand(1, 45, generator=g)
    lab = torch.randint(0, C, (1, 512, 512), generator=g)
    w = _yaml_weights()
    tr = flair_amd.SegTrainer(hip, lr=0.0, class_weight=w, metadata_encoder=enc)
    p0 = hip.flat_parameters().detach().clone()
    loss = float(tr.train_step(x.to(dev), lab.to(torch.uint8).to(dev), mtd.to(dev)))

    def oracle(net, mlp, xx, mm, ww):
        net.train(); net.zero_grad(); mlp.zero_grad()
        feats = net.encoder(xx)
        feats[-1] = torch.add(feats[-1], mlp(mm).unsqueeze(1).unsqueeze(-1).repeat(1, 512, 1, 16))
        l_ = nn.functional.cross_entropy(net.segmentation_head(net.decoder(*feats)), lab, weight=ww)
        l_.backward()
        return float(l_.detach()), {k: p.grad.detach().clone() for k, p in net.named_parameters()}, {k: p.grad.detach().clone() for k, p in mlp.named_parameters()}

    ref64, enc64 = copy.deepcopy(ref).double(), copy.deepcopy(enc_cpu).double()
    l32, g32, e32 = oracle(ref, enc_cpu, x, mtd, w)
    l64, g64, e64 = oracle(ref64, enc64, x.double(), mtd.double(), w.double())
    print(f"loss hip {loss:.7f} cpu fp32 {l32:.7f} fp64 {l64:.7f}")
    assert abs(loss - l64) <= 2e-4 * abs(l64) and abs(loss - l32) <= 2e-4 * abs(l32)
    hip_g = dict(zip(hip._param_names, [t.cpu() for t in hip._grad_views(tr.grads)]))
    assert_as_good_as_cpu_fp32(_tensor_errs(hip_g, g64), _tensor_errs(g32, g64), "grad_vs_fp64_rows_train_step_unet", (2.0, 2.5, 3.0))
    names = [k for k, _ in enc.named_parameters()]
    mlp_g = dict(zip(names, [t.cpu().view_as(e64[k]) for k, t in zip(names, tr.mlp_grads.split([e64[k].numel() for k in names]))]))
    assert_as_good_as_cpu_fp32(_tensor_errs(mlp_g, e64), _tensor_errs(e32, e64), "grad_vs_fp64_rows_train_step_mlp", (2.0, 2.5, 3.0))
    # lr = 0: nothing moved
    assert torch.equal(hip.flat_parameters(), p0)
    assert all(torch.equal(p.detach().cpu(), q.detach()) for p, q in zip(enc.parameters(), enc_cpu.parameters()))


def test_eval_steps_after_a_metadata_step_see_both_updates(dev):
    """The new writer against the eval caches: validate_step / predict with metadata before and after a train_step with metadata;
    afterwards they equal, bit for bit, a fresh model and a fresh encoder loaded from the two state_dict()s."""
    import flair_amd
    C = 19
    w = _yaml_weights()
    _, m = _pair(5, C, 41, dev)
    enc = _seeded_mlp(42).to(dev).eval()
    x, mtd, lab = _batch512(1, C, 15)
    x, mtd, lab = x.to(dev), mtd.to(dev), lab.to(torch.uint8).to(dev)
    tr = flair_amd.SegTrainer(m.train(), lr=0.05, class_weight=w, metadata_encoder=enc)
    before_loss = [tr.validate_step(x, lab, mtd).clone() for _ in range(3)][-1]     # (fills the eval caches, graph included)
    before_preds = [tr.predict(x, mtd).clone() for _ in range(3)][-1]
    tr.train_step(x, lab, mtd)
    after_loss = tr.validate_step(x, lab, mtd).clone()
    after_preds = tr.predict(x, mtd).clone()
    fresh = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=C, compute_dtype="f32")
    fresh.load_state_dict(m.state_dict(), strict=True)
    fresh_enc = flair_amd.MetadataMLP()
    fresh_enc.load_state_dict(enc.state_dict())
    tf = flair_amd.SegTrainer(fresh.to(dev).train(), lr=0.05, class_weight=w, metadata_encoder=fresh_enc.to(dev).eval())
    want_loss = tf.validate_step(x, lab, mtd)
    want_preds = tf.predict(x, mtd)
    assert torch.equal(_bits(after_loss), _bits(want_loss)), (float(after_loss), float(want_loss))
    assert torch.equal(after_preds, want_preds)
    assert not torch.equal(after_loss, before_loss) and not torch.equal(after_preds, before_preds)
    # the MLP's share of the update reaches the rows these steps add (the loss of this random network, near 40, does not resolve it)
    old_enc = _seeded_mlp(42).to(dev).eval()
    with torch.no_grad():
        assert not torch.equal(enc(mtd, masks=None), old_enc(mtd, masks=None))
        assert torch.equal(enc(mtd, masks=None), tf.metadata_encoder(mtd, masks=None))


def test_train_step_metadata_contract(dev):
    import flair_amd
    C = 13
    _, a = _pair(5, C, 5, dev)
    _, b = _pair(5, C, 5, dev)
    enc = _seeded_mlp(9).to(dev).train()
    enc0 = copy.deepcopy(enc)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 5, 64, 64, generator=g).to(dev)
    lab = torch.randint(0, C, (2, 64, 64), generator=g).to(torch.uint8).to(dev)
    mtd = torch.rand(2, 45, generator=g).to(dev)
    ta = flair_amd.SegTrainer(a.train(), lr=0.02, metadata_encoder=enc)
    tb = flair_amd.SegTrainer(b.train(), lr=0.02)
    with pytest.raises(ValueError, match="metadata_encoder"):
        tb.train_step(x, lab, mtd)
    with pytest.raises(RuntimeError, match="512x512"):
        ta.train_step(x, lab, mtd)
    start = a.flat_parameters().detach().clone()
    assert torch.equal(start, b.flat_parameters())               # the refused calls ran nothing
    la, lb = ta.train_step(x, lab), tb.train_step(x, lab)        # mtd=None with an encoder: the plain step
    assert torch.equal(_bits(la), _bits(lb))
    assert torch.equal(_bits(a.flat_parameters()), _bits(b.flat_parameters())) and not torch.equal(a.flat_parameters(), start)
    assert torch.equal(_bits(a.flat_buffers()), _bits(b.flat_buffers())) and torch.equal(a._flat_n, b._flat_n)
    assert _mlp_equal(enc, enc0) and ta.mlp_grads is None


# ------------------------------------------------------------------------------------------------ 4. two ranks on one GPU
DDP_LR = 0.05


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _ddp_model(seed):
    import flair_amd
    state = torch.random.get_rng_state()
    torch.manual_seed(seed)
    try:
        return flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=13, compute_dtype="f32")
    finally:
        torch.random.set_rng_state(state)


def _ddp_batch(rank):
    x, mtd, lab = _batch512(1, 13, 2022 + rank)
    return x, mtd, lab.to(torch.uint8)


def _ddp_worker(rank, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    import flair_amd
    dev = torch.device("cuda:0")
    model = _ddp_model(100 + rank).to(dev).train()          # different initial weights, U-Net and MLP: rank 0's must arrive
    enc = _seeded_mlp(200 + rank).to(dev).eval()             # dropout off
    tr = flair_amd.SegTrainer(model, lr=DDP_LR, metadata_encoder=enc)
    x, mtd, lab = (t.to(dev) for t in _ddp_batch(rank))
    loss = tr.train_step(x, lab, mtd)
    torch.cuda.synchronize()
    out[rank] = (model.flat_parameters().detach().cpu(), [p.detach().cpu() for p in enc.parameters()], float(loss), tr.mlp_grads.cpu())
    dist.destroy_process_group()


def test_two_ranks_with_metadata_match_single_process_average(dev):
    import flair_amd
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_ddp_worker, args=(r, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    (w0, e0, _, mg0), (w1, e1, _, mg1) = out[0], out[1]
    assert torch.equal(w0, w1) and all(torch.equal(p, q) for p, q in zip(e0, e1))     # replicas bit-identical, MLP included
    assert torch.equal(mg0, mg1)                                                       # the summed MLP gradient
    # single-process replay from rank 0's initial weights, gradients averaged by hand
    reps = [_ddp_model(100).to(dev).train() for _ in range(2)]
    encs = [_seeded_mlp(200).to(dev).eval() for _ in range(2)]
    trs = [flair_amd.SegTrainer(m, lr=0.0, metadata_encoder=e) for m, e in zip(reps, encs)]
    for r, t in enumerate(trs):
        x, mtd, lab = (v.to(dev) for v in _ddp_batch(r))
        t.train_step(x, lab, mtd)                              # lr = 0: gradients only
    mean = (trs[0].grads + trs[1].grads) / 2
    ref_w = (reps[0].flat_parameters().detach() - DDP_LR * mean).cpu()
    mlp_mean = (trs[0].mlp_grads + trs[1].mlp_grads) / 2
    ps = list(encs[0].parameters())
    ref_e = [(p.detach() - DDP_LR * g.view_as(p)).cpu() for p, g in zip(ps, mlp_mean.split([p.numel() for p in ps]))]
    err_w = float((w0 - ref_w).abs().max())
    err_e = max(float((p - q).abs().max()) for p, q in zip(e0, ref_e))
    print(f"max |weights - replay| U-Net {err_w:.3e} MLP {err_e:.3e}")
    assert err_w < 2e-6 and err_e < 2e-6       # (g0 + g1) * (lr / 2) vs ((g0 + g1) / 2) * lr: rounding only
    # the steps moved the weights, and rank 1 ended where rank 0's start leads, not its own
    start0 = [p.detach().cpu() for p in _seeded_mlp(200).parameters()]
    start1 = [p.detach().cpu() for p in _seeded_mlp(201).parameters()]
    moved = max(float((p - q).abs().max()) for p, q in zip(e1, start0))
    assert 0 < moved < 0.5 * min(float((p - q).abs().max()) for p, q in zip(start0, start1) if p.dim() == 2), moved
    assert float((w0 - _ddp_model(100).to(dev).flat_parameters().detach().cpu()).abs().max()) > 1e-4
