"""Exact-arithmetic operator tests: the HIP kernels on small-integer data against the fp64 CPU reference with torch.equal.

Activations, weights and gradients are in {-1, 0, 1}: every partial sum is an integer below 2^24, exact in fp32 in any summation
order, and every output is within +-256, exact in bf16 (tests/exact_cases.py asserts both on the reference alone).  One dropped,
doubled or misplaced term anywhere is a failure in either dtype.  The cases are sized so that persistent workgroups walk several
tiles unevenly, weight-gradient splits have remainders, reductions pass their block caps and the halo-GEMM's XCD remap runs with
a quotient and a remainder; each case asserts through the profile that the kernel family it is written for is the one that ran.

Both dtypes of a case share one reference (exact_cases caches the last two), so the dtype parameter varies fastest.  Nothing here
needs more than one process or 1 GB of device memory; the whole file takes well under a minute on an MI355X."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_cases as E
import launch_helpers as LH

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
TOL = {"f32": 2e-4, "bf16": 3e-2}   # test_gpu_ops.py's, for what goes through rsqrt


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _nhwc(x, dt, dev):
    return None if x is None else x.permute(0, 2, 3, 1).contiguous().to(device=dev, dtype=TDT[dt])


def _nchw(y):
    return y.float().cpu().permute(0, 3, 1, 2).double()


def _same(got, ref, what):
    """torch.equal with a message that says where."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {ref.numel()} elements differ, first at {i}: got {float(got[i])}, "
                             f"expected {float(ref[i])}; last at {tuple(int(v) for v in bad[-1])}")


_tuned = functools.partial(LH.tuned, defaults=E.TUNE_DEFAULTS)
_profiled = functools.partial(LH.profiled, keep=("conv", "wgrad"))   # the convolution and weight-gradient launches


# ------------------------------------------------------------------------------------------------ convolutions, plain entry points
@pytest.mark.parametrize("dt", E.DTYPES)
@pytest.mark.parametrize("case", E.CONV_CASES, ids=lambda c: c.name)
def test_conv_exact(dev, dt, case):
    from flair_amd import ops
    if dt not in case.dtypes:
        return
    ref = E.case_reference(case)
    E.check_exact_range(case, ref)
    E.check_dispatch_and_loops(case)
    x0, x1, w, b = ref["x0"], ref["x1"], ref["w"], ref["b"]
    with _tuned(case.tune):
        (y, yn, st), ran = _profiled(lambda: ops.conv2d_forward(
            _nhwc(x0, dt, dev), w.to(dev), bias=None if b is None else b.to(dev), stride=case.stride, pad=case.pad, x1=_nhwc(x1, dt, dev),
            up0=case.up0, want_nchw=case.nchw, want_stats=case.stats))
        assert ran == {case.fwd_kernel(dt)[1]: 1}, (case.name, dt, "forward ran", ran)
        if y is not None:
            _same(_nchw(y), ref["y"], "y (NHWC)")
        else:
            assert case.Cout % 8
        if case.nchw or y is None:
            _same(yn.cpu(), ref["y"], "y (fp32 NCHW copy)")
        if case.stats:
            _same(st.cpu(), torch.stack([ref["s1"], ref["s2"]]), "BatchNorm statistics (sum, sum of squares)")
        if not case.backward:
            return
        xin = E.assemble_input(x0, x1, case.up0)
        (dx, dw), ran = _profiled(lambda: ops.conv2d_backward(_nhwc(xin, dt, dev), w.to(dev), _nhwc(ref["dy"], dt, dev), stride=case.stride,
                                                              pad=case.pad, need_dx=case.need_dx))
        want = {case.dw_kernel(dt)[1]: 1}
        if case.need_dx:
            want[case.dx_kernel(dt)[1]] = 1
        assert ran == want, (case.name, dt, "backward ran", ran)
        if case.need_dx:
            _same(_nchw(dx), ref["dx"], "dx")
        _same(dw.cpu(), ref["dw"], "dw")


@pytest.mark.parametrize("dt", E.DTYPES)
def test_gather_wgrad_accumulates_into_a_prefilled_dw(dev, dt):
    """The 14-split gather-form case again through flair_conv2d_wgrad_ex with accumulate: wgrad_reduce_kernel adds its sum to what
    dw held (integers: exact)."""
    from flair_amd import ops
    case = next(c for c in E.CONV_CASES if c.name == E.WG_ACCUMULATE_CASE)
    ref = E.case_reference(case)
    E.check_wg_plan(case)
    prev = E.ints(tuple(ref["dw"].shape), torch.Generator().manual_seed(14), -64, 64)
    dw = prev.to(dev)
    _, ran = _profiled(lambda: ops.conv2d_wgrad_ex(_nhwc(ref["x0"], dt, dev), _nhwc(ref["dy"], dt, dev), case.Cout, stride=case.stride,
                                                   pad=case.pad, dw=dw, accumulate=True))
    assert ran == {case.dw_kernel(dt)[1]: 1}, ran
    _same(dw.cpu(), ref["dw"] + prev.double(), "dw += weight gradient")


# ------------------------------------------------------------------------------------------------ fused forms (flair_conv2d_ex / _wgrad_ex)
def _vec(t, dev):
    return None if t is None else t.to(dev)


@pytest.mark.parametrize("dt", E.DTYPES)
@pytest.mark.parametrize("case", E.FUSED_CASES, ids=lambda c: c.name)
def test_fused_forms_exact(dev, dt, case):
    """The options the network launches the convolutions with, through the operator entry points that expose them.
    argmax: maxprob_f32 is held to the 1e-6 that test_confmat_and_softmax_argmax applies to the standalone kernel's; both errors
    are printed (measured on an MI355X, integer logits: see the assertion message if it ever fails)."""
    from flair_amd import ops
    c = case
    r = E.fused_reference(c)
    E.check_fused_range(c, r)
    E.check_fused_dispatch_and_loops(c)
    x0, x1 = _nhwc(r["x0"], dt, dev), _nhwc(r["x1"], dt, dev)
    name = E.fused_kernel(c, dt)[1]
    with _tuned(c.tune):
        if c.kind in ("wgrad2", "wgrad_lazy", "dbias"):
            (dw, db), ran = _profiled(lambda: ops.conv2d_wgrad_ex(x0, _nhwc(r["dy"], dt, dev), c.Cout, x1=x1, up0=c.up0,
                                                                  in_scale=_vec(r.get("in_scale"), dev), in_shift=_vec(r.get("in_shift"), dev),
                                                                  want_dbias=c.kind == "dbias"))
            assert ran == {name: 1}, (c.name, dt, ran)
            _same(dw.cpu(), r["dw"], "dw")
            if c.kind == "dbias":
                _same(db.cpu(), r["dbias"], "dbias")
            return
        w = r["w"].to(dev)
        if c.kind == "lazy":
            o, ran = _profiled(lambda: ops.conv2d_ex(x0, w, in_scale=r["in_scale"].to(dev), in_shift=r["in_shift"].to(dev), want_stats=True))
            _same(_nchw(o["y"]), r["y"], "y of the lazy BatchNorm + ReLU input")
            _same(o["stats"].cpu(), torch.stack([r["s1"], r["s2"]]), "statistics")
        elif c.kind == "epilogue":
            kw = dict(bias=r["bias"].to(dev), oscale=r["oscale"].to(dev), oshift=r["oshift"].to(dev), ores=_nhwc(r["ores"], dt, dev))
            o, ran = _profiled(lambda: ops.conv2d_ex(x0, w, orelu=True, **kw))
            _same(_nchw(o["y"]), r["y"], "relu(acc * oscale + oshift + bias + ores)")
            o2, ran2 = _profiled(lambda: ops.conv2d_ex(x0, w, orelu=False, **kw))
            assert ran2 == ran
            _same(_nchw(o2["y"]), r["pre"], "acc * oscale + oshift + bias + ores")
        elif c.kind == "accumulate":
            out = _nhwc(r["prev"], dt, dev)
            o, ran = _profiled(lambda: ops.conv2d_ex(x0, w, mode=1, out=out, accumulate=True))
            _same(_nchw(o["y"]), r["y"], "out += data gradient")
        elif c.kind == "acc_src":
            src = _nhwc(r["prev"], dt, dev)
            o, ran = _profiled(lambda: ops.conv2d_ex(x0, w, mode=1, accumulate=True, acc_src=src))
            _same(_nchw(o["y"]), r["y"], "out = acc_src + data gradient")
            _same(_nchw(src), r["prev"], "acc_src is left alone")
        elif c.kind == "pool":
            skip = _nhwc(r["prev_skip"], dt, dev) if c.skip_accumulate else None
            o, ran = _profiled(lambda: ops.conv2d_ex(x0, w, mode=1, pool_c0=c.pool_c0, out_skip=skip, skip_accumulate=c.skip_accumulate))
            _same(_nchw(o["y"]), r["y"], "2x2 sum-pooled columns")
            if c.pool_c0 < c.Cout:
                _same(_nchw(o["out_skip"]), r["skip"], "skip columns")
        elif c.kind == "argmax":
            o, ran = _profiled(lambda: ops.conv2d_ex(x0, w, bias=r["bias"].to(dev), want_nhwc=False, want_preds=True, want_maxprob=True))
            _same(o["preds"].cpu(), r["preds"], "preds_u8 (first maximum)")
            err = float((o["maxprob"].cpu().double() - r["maxprob"]).abs().max())
            _, mp = ops.softmax_argmax(r["y"].float().to(dev), want="u8", want_maxprob=True)
            err_alone = float((mp.cpu().double() - r["maxprob"]).abs().max())
            print(f"{c.name} {dt}: max |maxprob - softmax_fp64| epilogue {err:.3e}, standalone flair_softmax_argmax {err_alone:.3e}")
            assert err < 1e-6, (err, err_alone)
        assert ran == {name: 1}, (c.name, dt, ran)


def test_fused_forms_refuse_what_the_kernel_does_not_implement(dev):
    """launch_conv's / launch_wgrad's own refusal (-6) comes back unchanged."""
    from flair_amd import ops
    from flair_amd._lib import FlairHipError
    g = torch.Generator().manual_seed(0)
    one = lambda n: torch.ones(n, device=dev)
    x = _nhwc(E.ternary((1, 64, 10, 12), g, 0.5), "f32", dev)             # not tileable: gather-form kernel
    w = E.ternary((64, 64, 3, 3), g, 0.5).to(dev)
    with pytest.raises(FlairHipError, match=r"code -6"):
        ops.conv2d_ex(x, w, in_scale=one(64), in_shift=one(64))
    x = _nhwc(E.ternary((1, 16, 16, 64), g, 0.5), "f32", dev)             # small-channel halo kernel: no acc_src, no partial pool
    w = E.ternary((16, 16, 3, 3), g, 0.5).to(dev)
    with pytest.raises(FlairHipError, match=r"code -6"):
        ops.conv2d_ex(x, w, mode=1, accumulate=True, acc_src=torch.zeros_like(x))
    x32 = _nhwc(E.ternary((1, 32, 16, 64), g, 0.5), "f32", dev)
    with pytest.raises(FlairHipError, match=r"code -6"):                  # dbias: 16 -> <= 16 layers only
        ops.conv2d_wgrad_ex(x32, x32, 32, want_dbias=True)
    with pytest.raises(FlairHipError, match=r"code -6"):                  # mode 1 is the stride-1 data gradient
        ops.conv2d_ex(x, w, mode=1, stride=2)


# ------------------------------------------------------------------------------------------------ reductions at their caps
@pytest.mark.parametrize("dt", E.DTYPES)
@pytest.mark.parametrize("shape", E.BN_CASES, ids=lambda s: "x".join(map(str, s)))
def test_bn_past_the_block_cap(dev, dt, shape):
    """rows > 2048 * 256 and not a multiple of 256: bn_bwd_blocks clamps and the reduction kernels grid-stride with a ragged tail.
    Integer y, gamma = 1, beta = 0: the batch sums are exact; dbeta = column sums of a ternary dout is exact."""
    from flair_amd import ops
    N, H, W, Cc = shape
    rows = N * H * W
    g = torch.Generator().manual_seed(Cc)
    y = E.ternary((rows, Cc), g, 0.5)
    y[:, 0] = 0
    y[0:2 * 100003:2, 0], y[1:2 * 100003:2, 0] = 1, -1       # channel 0: as many +1 as -1, its mean is exactly 0
    y[-1, 1] = 1                                             # the very last row counts (ragged tail)
    dout = E.ternary((rows, Cc), g, 0.5)
    yd, dd = y.double(), dout.double()
    s1 = yd.sum(0)
    assert float(yd.abs().sum(0).max()) < E.EXACT
    mean = s1 / rows
    var = (yd * yd).sum(0) / rows - mean * mean
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    xhat = (yd - mean) * invstd
    rm, rv = torch.zeros(Cc, device=dev), torch.ones(Cc, device=dev)
    ones, zeros = torch.ones(Cc, device=dev), torch.zeros(Cc, device=dev)
    yk = y.view(N, H, W, Cc).to(device=dev, dtype=TDT[dt])
    out, mean_k, invstd_k = ops.bn_relu_forward(yk, ones, zeros, rm, rv, training=True, relu=False)
    assert float(mean_k[0]) == 0.0
    assert _rel(mean_k.cpu(), mean) < 1e-5 and _rel(invstd_k.cpu(), invstd) < 1e-5
    assert _rel(rm.cpu(), 0.1 * mean) < 1e-5 and _rel(rv.cpu(), 0.9 + 0.1 * var * rows / (rows - 1)) < 1e-5
    assert _rel(out.float().cpu().view(rows, Cc), xhat) < TOL[dt]
    dk = dout.view(N, H, W, Cc).to(device=dev, dtype=TDT[dt])
    dy, _, dg, db = ops.bn_relu_backward(dk, out, yk, ones, mean_k, invstd_k, relu=False)
    _same(db.cpu(), dd.sum(0), "dbeta (integer column sums)")
    dg_ref = (dd * xhat).sum(0)
    assert _rel(dg.cpu(), dg_ref) < TOL[dt]
    dy_ref = invstd * (dd - dd.mean(0) - xhat * dg_ref / rows)
    assert _rel(dy.float().cpu().view(rows, Cc), dy_ref) < TOL[dt]


@pytest.mark.parametrize("dt", E.DTYPES)
@pytest.mark.parametrize("shape", E.POOL_CASES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_layer_sized_with_ties_everywhere(dev, dt, shape):
    from flair_amd import ops
    N, H, W, Cc = shape
    g = torch.Generator().manual_seed(H)
    x = torch.relu(E.ternary((N, Cc, H, W), g, 0.5)).double().requires_grad_(True)     # {0, 1}: every window has ties
    y = F.max_pool2d(x, 3, 2, 1)
    dy = E.ternary(tuple(y.shape), g, 0.5)
    y.backward(dy.double())
    yk, idx = ops.maxpool_forward(_nhwc(x.detach().float(), dt, dev))
    _same(_nchw(yk), y.detach(), "max pool")
    dx = ops.maxpool_backward(_nhwc(dy, dt, dev), idx, H, W)
    _same(_nchw(dx), x.grad, "max pool backward (the first maximum of a window takes the gradient)")


@functools.lru_cache(maxsize=1)
def _ce_oracle(shape, Cc):
    from oracle import seg_step
    B, H, W = shape
    g = torch.Generator().manual_seed(Cc + H)
    logits = E.ints((B, Cc, H, W), g, -3, 3)
    lab = torch.randint(0, Cc, (B, H, W), generator=g)
    w = torch.rand(Cc, generator=g) + 0.1
    w[2] = 0.0
    onehot = F.one_hot(lab, Cc).permute(0, 3, 1, 2).float().contiguous()
    onehot[0, :, :3, :3] = 0   # all-zero one-hot pixels -> class 0
    lab_eff = onehot.argmax(1)
    with torch.no_grad():
        loss_ref, preds_ref, targets_ref = seg_step.step_torch(logits, onehot, w)
    loss_np, dl_np = seg_step.cross_entropy_np(logits.numpy(), lab_eff.numpy(), w.numpy())
    cm_ref = seg_step.confusion_matrix_np(targets_ref.numpy(), preds_ref.numpy(), Cc)
    return logits, w, onehot, lab_eff, float(loss_ref), preds_ref, targets_ref, loss_np, dl_np, cm_ref


@pytest.mark.parametrize("kind", ["u8", "i64", "onehot"])
@pytest.mark.parametrize("Cc", [13, 19])
@pytest.mark.parametrize("shape", E.CE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ce_head_past_the_block_cap_and_on_the_scalar_kernel(dev, shape, Cc, kind):
    """9x512x512: the vec4 kernel grid-strides past its 2 048 blocks; H*W % 4 != 0: the scalar ce_main_kernel, small and past the
    cap.  Integer logits tie in most pixels: preds, targets and the confusion matrix equal the oracle's, first index winning;
    loss and dlogits keep the bounds of test_ce_head_against_oracle."""
    from flair_amd import ops
    logits, w, onehot, lab_eff, loss_ref, preds_ref, targets_ref, loss_np, dl_np, cm_ref = _ce_oracle(shape, Cc)
    labels = {"u8": lab_eff.to(torch.uint8), "i64": lab_eff, "onehot": onehot}[kind].to(dev)
    cm = torch.zeros(Cc, Cc, dtype=torch.int64, device=dev)
    loss, dl, preds, tg = ops.ce_head(logits.to(dev), labels, w.to(dev), want_preds="i64", confmat=cm, want_targets=True)
    assert torch.equal(preds.cpu().flatten(1), preds_ref)
    assert torch.equal(tg.cpu().flatten(1), targets_ref)
    assert np.array_equal(cm.cpu().numpy(), cm_ref)
    print(f"ce {shape} C={Cc} {kind}: loss {loss.item():.9f} fp64 {loss_np:.9f} torch {loss_ref:.9f}")
    assert abs(loss.item() - loss_np) < 2e-6 * max(1, abs(loss_np)) and abs(loss.item() - loss_ref) < 1e-5
    assert np.abs(dl.cpu().numpy() - dl_np).max() < 1e-9 + 1e-5 * np.abs(dl_np).max()


@pytest.mark.parametrize("shape,Cc", [(E.CE_SHAPES[0], 19), (E.CE_SHAPES[2], 13), (E.CE_SHAPES[1], 19)],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_softmax_argmax_and_confmat_past_the_block_cap(dev, shape, Cc):
    from flair_amd import _lib as L, ops
    from oracle import seg_step
    B, H, W = shape
    g = torch.Generator().manual_seed(Cc)
    logits = E.ints((B, Cc, H, W), g, -3, 3)
    pref = seg_step.predict_torch(logits)
    mref = torch.softmax(logits.double(), 1).max(1).values
    pr, mp = ops.softmax_argmax(logits.to(dev), want="i64", want_maxprob=True)
    assert torch.equal(pr.cpu(), pref)
    assert float((mp.cpu().double() - mref).abs().max()) < 1e-6
    # the network's own layout: NHWC rows of 16 / 32 columns
    ld = 16 if Cc <= 16 else 32
    for dt in E.DTYPES:
        lg = torch.zeros(B, H, W, ld)
        lg[..., :Cc] = logits.permute(0, 2, 3, 1)
        lg = lg.to(device=dev, dtype=TDT[dt])
        pu8 = torch.empty(B, H, W, dtype=torch.uint8, device=dev)
        mp2 = torch.empty(B, H, W, dtype=torch.float32, device=dev)
        L.check(L.lib().flair_softmax_argmax_nhwc(L.ptr(lg), L.dtype_code(TDT[dt]), ld, B, Cc, H, W, L.ptr(pu8), None, L.ptr(mp2), L.stream()))
        assert torch.equal(pu8.cpu().long(), pref)
        assert float((mp2.cpu().double() - mref).abs().max()) < 1e-6
    t = torch.randint(0, Cc, (B * H * W,), generator=g, dtype=torch.int32)
    p = torch.randint(0, Cc, (B * H * W,), generator=g)
    cm = ops.confmat_update(torch.zeros(Cc, Cc, dtype=torch.int64, device=dev), t.to(dev), p.to(dev))
    assert np.array_equal(cm.cpu().numpy(), seg_step.confusion_matrix_np(t.numpy(), p.numpy(), Cc))


# ------------------------------------------------------------------------------------------------ the trainer's SGD
# p in [-64, 64], g in [-8, 8], lr = 0.25: lr * g is a multiple of 1/4 within +-2 and p - lr * g one within +-66, both exact in fp32
# whether or not the compiler contracts them into an FMA.  4 096 blocks of 256 threads take 4 floats each per pass: 4 194 304 elements;
# the last length makes three passes, the third over 777 float4s, and leaves a 3-element tail.
SGD_LENGTHS = [1, 2, 3, 4, 7, 4097, 2 * 4096 * 256 * 4 + 4 * 777 + 3]
SGD_PAD = 8          # floats after the n updated ones, in the same allocation


@pytest.mark.parametrize("n", SGD_LENGTHS)
def test_sgd_step_exact_over_loop_passes_tails_and_padding(dev, n):
    from flair_amd import _lib as L
    assert SGD_LENGTHS[-1] == 8388608 + 4 * 777 + 3
    g = torch.Generator().manual_seed(n % 1000)
    p = torch.randint(-64, 65, (n + SGD_PAD,), generator=g).float()
    gr = torch.randint(-8, 9, (n + SGD_PAD,), generator=g).float()
    want = p.double()
    want[:n] -= 0.25 * gr[:n].double()
    assert torch.equal(want.float().double(), want)      # the expectation is an fp32 number
    pd, gd = p.to(dev), gr.to(dev)
    assert L.lib().flair_sgd_step(L.ptr(pd), L.ptr(gd), n, 0.25, L.stream()) == 0
    got = pd.cpu()
    bad = int((got[:n].double() != want[:n]).sum())
    assert bad == 0, f"n={n}: {bad} elements differ"
    assert torch.equal(got[n:], p[n:])                   # nothing past n is written, whatever n is modulo 4
    assert torch.equal(gd.cpu(), gr)


def test_sgd_step_refuses_a_pointer_that_is_not_16_byte_aligned(dev):
    from flair_amd import _lib as L
    p = torch.arange(16, dtype=torch.float32, device=dev)
    g = torch.ones(16, dtype=torch.float32, device=dev)
    before = p.clone()
    assert L.lib().flair_sgd_step(p.data_ptr() + 4, L.ptr(g), 8, 0.25, L.stream()) == -2
    assert L.lib().flair_sgd_step(L.ptr(p), g.data_ptr() + 4, 8, 0.25, L.stream()) == -2
    assert L.lib().flair_sgd_step(None, L.ptr(g), 8, 0.25, L.stream()) == -1
    assert torch.equal(p, before)
