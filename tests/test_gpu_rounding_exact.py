"""Exact tests for where the bf16 U-Net kernels round: the HIP kernels on "integer-beyond-256" data (tests/rounding_cases.py) against
the fp64 CPU reference with the bf16 rounding applied at exactly the points the code documents, compared with torch.equal.

Inputs are bf16 values, every accumulation is exact in fp32 in any order, and the results need more than 8 significant bits: every
bf16 store rounds, so a kernel that took BatchNorm statistics or partial sums from unrounded values, rounded once where store_tile
rounds twice (or twice where bn_act rounds once), or truncated instead of rounding to nearest-even, fails here.  In fp32 the same
cases run with the rounding replaced by the identity: nothing may round there.  test_rounding_cases_cpu.py asserts on the
references alone that the cases are inside the exact range and tell the right placement from the wrong ones.

Forms (DESIGN.md "Where bf16 rounds"): a. forward per family with statistics and the head's fp32 NCHW copy, b. inference epilogue,
c. data-gradient forms (accumulate, acc_src, pool_c0, fused BatchNorm-backward sums, parity-class stride 2), d. lazy BatchNorm +
ReLU input (forward and weight gradient), e. the stem weight gradient's fused apply, f. the elementwise kernels.  Every
convolution / weight-gradient test asserts through the launch profile that the family it is written for ran, once.

One or two tiles per case, at most 512 output pixels; one process, a few MB of device memory; the 98 tests of this file take 3.4 s on
an MI355X (the slowest 0.8 s)."""
import pytest
import torch
import torch.nn.functional as F

import bwd_fused_cases as B
import exact_cases as E
import rounding_cases as R
from test_gpu_bwd_fused_exact import NAN, SENTINEL, TDT, _backed, _nchw, _nhwc, _profiled, _same, _tuned

pytestmark = pytest.mark.gpu


def _convs(ran):
    """the convolution / weight-gradient launches of a profile"""
    return {k: v for k, v in ran.items() if k.startswith(("conv", "wgrad"))}


def _filled(shape, dt, dev):
    return torch.full(shape, SENTINEL, dtype=TDT[dt], device=dev)


# ------------------------------------------------------------------------------------------------ a, b, c (plain), d (forward)
@pytest.mark.parametrize("dt", E.DTYPES)
@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: c.name)
def test_conv_rounding_exact(dev, dt, case):
    from flair_amd import ops
    c, r = case, R.conv_reference(case)
    want = R.conv_expect(c, r, R.ROUND[dt])
    name = c.launch(dt)[1]
    x, w = _nhwc(r["x"], dt, dev), r["w"].to(dev)
    vec = lambda k: r[k].to(dev)
    with _tuned(()):
        if c.form == "fwd":
            (y, yn, st), ran = _profiled(lambda: ops.conv2d_forward(x, w, bias=vec("bias") if c.bias else None, stride=c.stride, pad=c.pad,
                                                                    want_nchw=c.nchw, want_stats=c.stats))
            if y is not None:
                _same(_nchw(y), want["y"], "y = rf(acc [+ bias])")
            if c.nchw or y is None:
                _same(yn, want["y"], "the fp32 NCHW copy holds the rounded values")
            if c.stats:
                _same(st, torch.stack([want["s1"], want["s2"]]), "statistics: sum and sum of squares of the ROUNDED outputs")
        elif c.form == "epilogue":
            kw = dict(bias=vec("bias"), oscale=vec("oscale"), oshift=vec("oshift"), ores=_nhwc(r["ores"], dt, dev))
            o, ran = _profiled(lambda: ops.conv2d_ex(x, w, orelu=True, **kw))
            _same(_nchw(o["y"]), want["y_relu"], "rf(relu(rf(acc oscale + oshift + bias) + ores))")
            o2, ran2 = _profiled(lambda: ops.conv2d_ex(x, w, orelu=False, **kw))
            assert _convs(ran2) == _convs(ran)
            _same(_nchw(o2["y"]), want["y_lin"], "rf(rf(acc oscale + oshift + bias) + ores)")
        elif c.form == "accumulate":
            out = _nhwc(r["prev"], dt, dev)
            _, ran = _profiled(lambda: ops.conv2d_ex(x, w, mode=1, out=out, accumulate=True))
            _same(_nchw(out), want["y"], "rf(rf(acc) + prev)")
        elif c.form == "acc_src":
            src, out = _nhwc(r["prev"], dt, dev), _filled((c.N, c.H, c.W, c.Cout), dt, dev)
            _, ran = _profiled(lambda: ops.conv2d_ex(x, w, mode=1, out=out, accumulate=True, acc_src=src))
            _same(_nchw(out), want["y"], "rf(rf(acc) + acc_src)")
        elif c.form == "pool":
            def fresh():
                out = _nhwc(r["prev"], dt, dev) if c.accumulate else _filled((c.N, c.H // 2, c.W // 2, c.pool_c0), dt, dev)
                skip = None
                if c.pool_c0 < c.Cout:
                    skip = _nhwc(r["prev_skip"], dt, dev) if c.skip_accumulate else _filled((c.N, c.H, c.W, c.Cout - c.pool_c0), dt, dev)
                return out, skip
            out, skip = fresh()
            _, ran = _profiled(lambda: ops.conv2d_ex(x, w, mode=1, pool_c0=c.pool_c0, out=out, accumulate=c.accumulate, out_skip=skip,
                                                     skip_accumulate=c.skip_accumulate))
            _same(_nchw(out), want["y"], "pooled columns: rf(((rf(a0) + rf(a1)) + rf(a2)) + rf(a3) [+ prev])")
            if skip is not None:
                _same(_nchw(skip), want["skip"], "skip columns: rf(acc) or rf(rf(acc) + prev_skip)")
            # the separate pass the epilogue replaces, on the materialised rf(acc): the same bits
            full = ops.conv2d_ex(x, w, mode=1)["y"]
            _same(_nchw(full), R.ROUND[dt](r["acc"]), "rf(acc)")
            out2, skip2 = fresh()
            _, ran_u = _profiled(lambda: ops.upcat_bwd(full, c.pool_c0, dx0=out2, dx0_accumulate=c.accumulate, dskip=skip2,
                                                       dskip_accumulate=c.skip_accumulate))
            assert ran_u == {"upcat_bwd": 1}, ran_u
            assert torch.equal(out, out2) and (skip is None or torch.equal(skip, skip2)), "upcat_bwd of rf(acc) and the pool_c0 epilogue differ"
        else:
            assert c.form == "lazy"
            o, ran = _profiled(lambda: ops.conv2d_ex(x, w, in_scale=vec("in_scale"), in_shift=vec("in_shift")))
            _same(_nchw(o["y"]), want["y"], "rf(conv(x')), x' = rf(relu(fmaf(x, s, sh)))")
            act, ran_a = _profiled(lambda: ops.bn_act(x, vec("in_scale"), vec("in_shift")))
            assert ran_a == {"bn_act": 1}, ran_a
            _same(_nchw(act), want["xp"], "bn_act: x'")
            assert torch.equal(o["y"], ops.conv2d_ex(act, w)["y"]), "the lazy input and bn_act + the plain form differ"
    assert _convs(ran) == {name: 1}, (c.name, dt, ran)


# ------------------------------------------------------------------------------------------------ c. fused BatchNorm-backward sums
@pytest.mark.parametrize("dt", E.DTYPES)
@pytest.mark.parametrize("case", R.BNR_CASES, ids=lambda c: c.name)
def test_bnr_sums_are_of_the_stored_gradient(dev, dt, case):
    from flair_amd import ops
    c, r = case, R.bnr_reference(case)
    want = R.bnr_expect(c, r, R.ROUND[dt])
    x, w = _nhwc(r["x"], dt, dev), r["w"].to(dev)
    full = c.N * c.H * c.W * c.Cout
    y = _backed(r["y"], dt, dev, full)
    bout = _backed(r["out"], dt, dev, full) if c.from_out else None
    shape = (c.N, c.H // 2, c.W // 2, c.pool_c0) if c.pool_c0 else (c.N, c.H, c.W, c.Cout)
    src = None
    if c.accumulate and not c.acc_src:
        out = _nhwc(r["prev"], dt, dev)
    else:
        out = _filled(shape, dt, dev)
        src = _nhwc(r["prev"], dt, dev) if c.acc_src else None
    skip = None
    if c.pool_c0 and c.pool_c0 < c.Cout:
        skip = _nhwc(r["prev_skip"], dt, dev) if c.skip_accumulate else _filled((c.N, c.H, c.W, c.Cout - c.pool_c0), dt, dev)
    kw = dict(mode=1, out=out, accumulate=c.accumulate, acc_src=src, pool_c0=c.pool_c0, out_skip=skip, skip_accumulate=c.skip_accumulate,
              bnr_y=y, bnr_out=bout, bnr_scale=r["scale"].to(dev), bnr_shift=r["shift"].to(dev), bnr_mask=c.bnr_mask)
    with _tuned(c.tune):
        rows = ops.conv2d_ex_grid_rows(x, w, **kw)
        assert rows == c.grid_rows(dt), (c.name, dt, rows)
        partial = torch.full((2, c.Cy, rows), NAN, dtype=torch.float32, device=dev)
        _, ran = _profiled(lambda: ops.conv2d_ex(x, w, bnr_partial=partial, **kw))
    assert _convs(ran) == {c.launch(dt)[1]: 1}, (c.name, dt, ran)
    _same(_nchw(out), want["stored"], "the stored gradient d (d m with bnr_mask)")
    if skip is not None:
        _same(_nchw(skip), want["skip"], "skip columns")
    _same(partial.double().sum(2), torch.stack([want["s1"], want["s2"]]), "(sum d m, sum d m y) of the STORED gradient")


@pytest.mark.parametrize("dt", E.DTYPES)
def test_parity_dgrad_accumulate_rounds_twice(dev, dt):
    from flair_amd import ops
    c, r = R.PARITY_CASE, R.parity_reference()
    dx = _nhwc(r["prev"], dt, dev)
    _, ran = _profiled(lambda: ops.conv2d_ex(_nhwc(r["dy"], dt, dev), r["w"].to(dev), mode=2, stride=2, pad=1, out=dx, accumulate=True))
    assert ran == {c.launch(dt)[1]: 1, "pack_weights_all": 1}, ran
    _same(_nchw(dx), R.parity_expect(r, R.ROUND[dt]), "rf(rf(acc) + prev)")


# ------------------------------------------------------------------------------------------------ d. lazy input of the weight gradient
@pytest.mark.parametrize("dt", E.DTYPES)
@pytest.mark.parametrize("case", R.WLAZY_CASES, ids=lambda c: c.name)
def test_wgrad_lazy_input_rounds_like_bn_act(dev, dt, case):
    from flair_amd import ops
    c, r = case, R.wlazy_reference(case)
    x, dy = _nhwc(r["x"], dt, dev), _nhwc(r["dy"], dt, dev)
    s, sh = r["in_scale"].to(dev), r["in_shift"].to(dev)
    with _tuned(c.tune):
        (dw, _), ran = _profiled(lambda: ops.conv2d_wgrad_ex(x, dy, c.Cout, in_scale=s, in_shift=sh))
        assert _convs(ran) == {E.fused_kernel(c, dt)[1]: 1}, (c.name, dt, ran)
        _same(dw, R.wlazy_expect(c, r, R.ROUND[dt]), "dw against x' = rf(relu(fmaf(x, s, sh)))")
        plain, _ = ops.conv2d_wgrad_ex(ops.bn_act(x, s, sh), dy, c.Cout)
    assert torch.equal(dw, plain), "the lazy input and bn_act + the plain form differ"


# ------------------------------------------------------------------------------------------------ e. stem weight gradient, fused apply
def _stem_inputs(dev):
    r = R.stem_reference()
    return r, tuple(_nhwc(r[k], "bf16", dev) for k in ("x", "dout", "y"))


def test_stem_fused_apply_rounds_the_staged_gradient(dev):
    """bf16 only (the stem kernels exist in bf16).  Coefficients in eighths: staged = rne(k1 dout m + k2 y + k3) needs more than 8
    bits, dw is the exact weight gradient against it, and the plain kernel on the materialised staged tensor gives the same bits."""
    from flair_amd import ops
    r, (x, dout, y) = _stem_inputs(dev)
    name = B.check_stem_dispatch(R.STEM_SHAPE)[1]
    dw = torch.full((64, 5, 7, 7), NAN, device=dev)
    _, ran = _profiled(lambda: ops.conv2d_wgrad_ex(x, dout, 64, R=7, stride=2, pad=3, cin_real=5, dw=dw, fuse_y=y, fuse_coef=r["coef"].to(dev),
                                                   fuse_msc=r["scale"].to(dev), fuse_msh=r["shift"].to(dev)))
    assert _convs(ran) == {name: 1}, ran
    _same(dw, R.stem_expect(r, R.rne), "dw against staged = rne(k1 dout m + k2 y + k3)")
    dw2, _ = ops.conv2d_wgrad_ex(x, _nhwc(R.rne(r["pre"]).float(), "bf16", dev), 64, R=7, stride=2, pad=3, cin_real=5)
    assert torch.equal(dw, dw2)


def test_stem_fused_apply_matches_bn_backward_then_the_plain_kernel(dev):
    """The two-launch form on the same data: bn_backward_ex writes dy (bn_bwd_apply: fmaf(k1, dm, fmaf(k2, y, k3)), one store), the
    plain stem kernel reads it; the fused kernel applies the coefficients bn_backward_ex left while it stages.  The same bits."""
    from flair_amd import ops
    r, (x, dout, y) = _stem_inputs(dev)
    mean, invstd, gamma = (t.to(dev) for t in B.bn_params(B._gen("rstem chain"), 64))
    msc, msh = r["scale"].to(dev), r["shift"].to(dev)
    rows2d = lambda t: t.reshape(-1, 64)
    both, ran = _profiled(lambda: ops.bn_backward_ex(rows2d(dout), rows2d(y), mean, invstd, gamma=gamma, mscale=msc, mshift=msh))
    assert ran == {"bn_bwd_reduce": 1, "bn_bwd_finalize": 1, "bn_bwd_apply": 1}, ran
    only = ops.bn_backward_ex(rows2d(dout), rows2d(y), mean, invstd, gamma=gamma, mscale=msc, mshift=msh, want_dy=False)
    assert torch.equal(only["coef"], both["coef"])
    fused, ran = _profiled(lambda: ops.conv2d_wgrad_ex(x, dout, 64, R=7, stride=2, pad=3, cin_real=5, fuse_y=y, fuse_coef=only["coef"],
                                                       fuse_msc=msc, fuse_msh=msh))
    assert _convs(ran) == {"wgrad_stem_bf16": 1}, ran
    plain, _ = ops.conv2d_wgrad_ex(x, both["dy"].view_as(dout), 64, R=7, stride=2, pad=3, cin_real=5)
    assert torch.equal(fused[0], plain), float((fused[0] - plain).abs().max())
    assert float(plain.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ f. elementwise
@pytest.mark.parametrize("dt", E.DTYPES)
def test_bn_act_rounds_once(dev, dt):
    from flair_amd import ops
    r, rf = R.elementwise_reference(), R.ROUND[dt]
    y, sc, sh = _nhwc(r["y"], dt, dev), r["scale"].to(dev), r["shift"].to(dev)
    for relu in (True, False):
        out, ran = _profiled(lambda: ops.bn_act(y, sc, sh, relu=relu))
        assert ran == {"bn_act": 1}, ran
        _same(_nchw(out), rf(torch.relu(r["pre"]) if relu else r["pre"]), f"rf([relu]fmaf(y, s, sh)), relu {relu}")
    # eval-mode BatchNorm + residual + ReLU: the scale is gamma / sqrt(running_var + eps) with an exact square root
    out, _, _ = ops.bn_relu_forward(y, r["gamma"].to(dev), r["beta"].to(dev), r["rm"].to(dev), r["rv"].to(dev), training=False,
                                    residual=_nhwc(r["res"], dt, dev), relu=True)
    _same(_nchw(out), rf(torch.relu(r["pre_res"])), "rf(relu(fmaf(y, sc, sh) + res))")


@pytest.mark.parametrize("dt", E.DTYPES)
def test_bn_act_maxpool_pools_the_rounded_activation(dev, dt):
    from flair_amd import ops
    r, rf = R.elementwise_reference(), R.ROUND[dt]
    y, sc, sh = _nhwc(r["ymp"], dt, dev), r["scale"].to(dev), r["shift"].to(dev)
    (act, pooled, idx), ran = _profiled(lambda: ops.bn_act_maxpool(y, sc, sh))
    assert ran == {"bn_act_maxpool": 1}, ran
    act2 = ops.bn_act(y, sc, sh)
    pooled2, idx2 = ops.maxpool_forward(act2)
    assert torch.equal(act, act2) and torch.equal(pooled, pooled2) and torch.equal(idx, idx2)
    a = rf(torch.relu(r["pre_mp"]))
    _same(_nchw(act), a, "rf(relu(fmaf(y, s, sh)))")
    _same(_nchw(pooled), F.max_pool2d(a, 3, 2, 1), "max pool of the ROUNDED activation")
    win = R.rounding_ties(r["pre_mp"])[1](a)
    first = (win == win.amax(4, keepdim=True)).double().argmax(4)
    _same(idx.permute(0, 3, 1, 2), first, "tap of the first maximum among the ROUNDED values (rounding makes ties)")


@pytest.mark.parametrize("dt", E.DTYPES)
def test_elementwise_accumulates_round_once(dev, dt):
    from flair_amd import ops
    r, rf = R.elementwise_reference(), R.ROUND[dt]
    N, H, W, Cc = R.EW_SHAPE
    a, b = r["a"].double(), r["b"].double()
    # ew_add_
    d = _nhwc(r["a"], dt, dev)
    ops.ew_add_(d, _nhwc(r["b"], dt, dev))
    _same(_nchw(d), rf(a + b), "ew_add_: rf(dst + src)")
    # bn_backward_ex, the residual gradient accumulated: dres = rf(prev + dout m); dbeta = sum dout m is exact
    flat = lambda t: _nhwc(t, dt, dev).reshape(-1, Cc)
    dres = flat(r["a"])
    got, ran = _profiled(lambda: ops.bn_backward_ex(flat(r["b"]), flat(r["bn_y"]), r["bn_mean"].to(dev), r["bn_invstd"].to(dev),
                                                    gamma=r["bn_gamma"].to(dev), out=flat(r["bn_out"]), dres=dres, dres_accumulate=True))
    assert ran == {"bn_bwd_reduce": 1, "bn_bwd_finalize": 1, "bn_bwd_apply": 1}, ran
    _same(_nchw(got["dres"].view(N, H, W, Cc)), rf(a + b * r["bn_m"]), "dres = rf(prev + dout m)")
    _same(got["dbeta"], (b * r["bn_m"]).sum(dim=(0, 2, 3)), "dbeta")
    # maxpool_backward_ex accumulate
    _, idx = ops.maxpool_forward(_nhwc(r["pool_x"], dt, dev))
    din = _nhwc(r["a"], dt, dev)
    _, ran = _profiled(lambda: ops.maxpool_backward_ex(_nhwc(r["pool_dy"], dt, dev), idx, H, W, dx=din, accumulate=True))
    assert ran == {"maxpool_bwd": 1}, ran
    _same(_nchw(din), rf(a + r["pool_dx"]), "din = rf(prev + max pool backward)")
    # upcat_bwd, all accumulate combinations: dx0 = rf(sum of four [+ prev]), dskip = dcat or rf(dcat + prev)
    C0 = Cc // 2
    p0, p1 = r["b"][:, :C0, ::2, ::2].contiguous(), r["b"][:, C0:].contiguous()
    dk = _nhwc(r["a"], dt, dev)
    s4 = R._sum4(a[:, :C0])
    for a0, a1 in ((False, False), (False, True), (True, False), (True, True)):
        dx0 = _nhwc(p0, dt, dev) if a0 else _filled((N, H // 2, W // 2, C0), dt, dev)
        dsk = _nhwc(p1, dt, dev) if a1 else _filled((N, H, W, Cc - C0), dt, dev)
        _, ran = _profiled(lambda: ops.upcat_bwd(dk, C0, dx0=dx0, dx0_accumulate=a0, dskip=dsk, dskip_accumulate=a1))
        assert ran == {"upcat_bwd": 1}, ran
        _same(_nchw(dx0), rf(s4 + (p0.double() if a0 else 0)), f"dx0 (accumulate {a0}, {a1})")
        _same(_nchw(dsk), rf(a[:, C0:] + (p1.double() if a1 else 0)), f"dskip (accumulate {a0}, {a1})")
