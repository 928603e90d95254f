"""Operator tests of the SegFormer / UperNet-Swin kernels (csrc/segformer_ops.hip, csrc/swin_ops.hip and the GEMM epilogues
they use) through the flair_sf_* / flair_swin_* entry points, against the fp64 references of tests/transformer_cases.py.

Three kinds of assertion:
  exact    torch.equal against fp64 where the arithmetic is exact by construction (attention as a gather, the decode head on
           dyadic data, dyadic resizes, power-of-two pools, ternary GEMMs, the elementwise kernels past their grid cap);
  derived  a bound worked out from the arithmetic where an exact pre-activation is followed by one known function (GELU) or a
           short fp32 expression (non-dyadic resizes and pools);
  measured where a reciprocal square root or a real softmax is involved: the error against the fp64 reference (never against
           another run of a kernel), relative to the reference's largest magnitude, is printed and logged through
           oracle.parity.record; the bound of a group is 3x its value in MEASURED below — the margin of the project's bf16
           network bounds; it covers another seed's worst element, not another algorithm — and never above the standing operator
           tolerances (2e-4 fp32, 3e-2 bf16).

tests/test_transformer_ops_cases_cpu.py asserts, on the references alone, that the exact cases are exact and that the loop cases
loop.  Every test takes a few seconds at most and well under 1 GB."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

import transformer_cases as T

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
U = 2.0 ** -24

# max |kernel - fp64 reference| / max |reference| over the cases of the group as measured on an MI355X (the log of that run
# is profiles/transformer_ops_parity.json, written with FLAIR_PARITY_JSON set); the bound of a group is 3x this
MEASURED = {
    ("sf_layernorm", "f32"): 9.966e-06, ("sf_layernorm", "bf16"): 3.084e-03,
    ("swin_layernorm", "f32"): 1.071e-05, ("swin_layernorm", "bf16"): 3.482e-03,
    ("swin_patch_merge_ln", "f32"): 1.482e-07, ("swin_patch_merge_ln", "bf16"): 3.397e-03,
    ("swin_window_attention", "f32"): 4.218e-07, ("swin_window_attention", "bf16"): 2.892e-03,
    ("sf_attention", "f32"): 1.081e-06, ("sf_attention", "bf16"): 2.852e-03, ("sf_attention_one_tile", "bf16"): 2.852e-03,
    ("sf_ffn_fused", "bf16"): 3.106e-03, ("sf_ffn_fused_ln", "bf16"): 1.938e-03,
}


def _ops():
    from flair_amd import ops
    return ops


def _to(x, dt, dev):
    return None if x is None else x.to(device=dev, dtype=TDT[dt]).contiguous()


def _f32(x, dev):
    return None if x is None else x.to(device=dev, dtype=torch.float32).contiguous()


def _back(y):
    return y.float().cpu().double()


def _same(got, ref, what):
    """torch.equal with a message that says where."""
    got, ref = _back(got) if got.is_cuda else got.double(), ref.double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {ref.numel()} elements differ, first at {i}: got {float(got[i])}, "
                             f"expected {float(ref[i])}; last at {tuple(int(v) for v in bad[-1])}")


def _within(got, ref, bound, what):
    """elementwise |got - ref| <= bound (a tensor)"""
    err = (_back(got) - ref).abs()
    over = err > bound
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: worst error / bound = {worst:.3f}")
    if bool(over.any()):
        i = tuple(int(v) for v in over.nonzero()[0])
        raise AssertionError(f"{what}: {int(over.sum())} of {ref.numel()} elements over their bound, first at {i}: got "
                             f"{float(_back(got)[i])}, expected {float(ref[i])}, bound {float(bound[i]):.3e}; worst ratio {worst:.2f}")


def _measured(group, dt, case, got, ref):
    """relative-to-maximum error against the fp64 reference: printed, logged, then asserted against 3x the measured value"""
    from oracle import parity
    err = float((_back(got) - ref).abs().max() / ref.abs().max())
    bound = 3 * MEASURED[(group, dt)]
    print(f"{group}[{dt}] {case}: rel err {err:.3e} (bound {bound:.3e})")
    parity.record({"test": f"transformer_ops/{group}/{dt}/{case}", "rel_err_vs_fp64": err, "bound": bound})
    assert bound <= T.TOL[dt]
    assert err <= bound, (group, dt, case, err, bound)
    return err


@contextlib.contextmanager
def _tuned(**pairs):
    from flair_amd import _lib as L
    try:
        for k, v in pairs.items():
            L.check(L.lib().flair_tune_set(k.encode(), v))
        yield
    finally:
        for k, v in T.TUNE_DEFAULTS.items():
            L.lib().flair_tune_set(k.encode(), v)


# ================================================================================================ exact: attention as a gather
@pytest.mark.parametrize("case", T.SF_GATHER_CASES, ids=lambda c: c[0])
def test_sf_attention_gathers_exactly(dev, case):
    """Every address and lane permutation of the three attention kernels, the key <-> value pairing of the accumulator-as-operand
    product included: the output row must be V[target] bit for bit.  The walk* cases reach qblocks > 1 (the multi-block walk, the
    prefetch of the next block's queries, the `q0 >= N` break and the clamp of a ragged tail inside a walked block)."""
    name, dt, att2, B, heads, N, Nk, _ = case
    q, kv, want, _ = T.sf_gather_inputs(case)
    hid = 64 * heads
    kvd = _to(kv, dt, dev)
    with _tuned(FLAIR_SF_ATT2=att2):
        out = _ops().sf_attention(_to(q, dt, dev), kvd[..., :hid], kvd[..., hid:], kv_ld=2 * hid)
    _same(out, want, f"sf_attention {name}")


@pytest.mark.parametrize("dt", T.DTYPES)
@pytest.mark.parametrize("case", T.SWIN_GATHER_CASES, ids=lambda c: c[0])
def test_swin_attention_gathers_exactly(dev, case, dt):
    """pad, roll, window split, merge back and crop of the shifted-window attention on grids smaller than, equal to and larger
    than a window, with both block parities: the output row must be V[target] bit for bit"""
    name, B, H, W, heads, shift = case
    qkv, bias, want, _ = T.swin_gather_inputs(case)
    table = torch.zeros(169, heads)
    out = _ops().swin_window_attention(_to(qkv, dt, dev), _f32(bias, dev), _f32(table, dev), heads, shift)
    _same(out, want, f"swin_window_attention {name} {dt}")


@pytest.mark.parametrize("dt", T.DTYPES)
@pytest.mark.parametrize("case", [c for c in T.SWIN_GATHER_CASES if c[0] in T.SWIN_MASK_NAMES], ids=lambda c: c[0])
def test_swin_attention_mask_is_minus_100(dev, case, dt):
    """a decoy key of another region with a raw advantage of 50 must lose to the -100 mask, one with 150 must win: the library's
    mask is -100, not -inf, and it is applied between regions only"""
    name, B, H, W, heads, shift = case
    qkv, bias, want, ndec = T.swin_gather_inputs(case, decoys=True)
    assert ndec[0] >= 1 and ndec[1] >= 1
    out = _ops().swin_window_attention(_to(qkv, dt, dev), _f32(bias, dev), _f32(torch.zeros(169, heads), dev), heads, shift)
    _same(out, want, f"swin_window_attention mask {name} {dt}")


# ===================================================================================================== exact: fused decode head
@pytest.mark.parametrize("case", T.HEAD_CASES, ids=str)
def test_head_fused_and_upsample_sum_are_exact(dev, case):
    H, W, D, labels = case
    d = T.head_inputs(case)
    z, logits = T.check_head_exact(d)
    ops = _ops()
    assert ops.sf_head_fused_ok("bf16", H, W, 64, D, labels)
    b = {k: _to(d[k], "bf16", dev) for k in ("f0", "g1", "g2", "g3")}
    out = ops.sf_head_fused(b["f0"], _f32(d["w0"], dev), b["g1"], b["g2"], b["g3"], _f32(d["scale"], dev), _f32(d["shift2"], dev),
                            _f32(d["wc"], dev), _f32(d["bc"], dev))
    _same(out, logits, f"sf_head_fused {case}")
    g0 = d["f0"] @ d["w0"].T
    for dt in T.DTYPES:
        zz = ops.sf_upsample_sum_bn_relu(_to(g0, dt, dev), _to(d["g1"], dt, dev), _to(d["g2"], dt, dev), _to(d["g3"], dt, dev),
                                         _f32(d["scale"], dev), _f32(d["shift2"], dev))
        _same(zz, z, f"sf_upsample_sum_bn_relu {case} {dt}")


def test_head_refusals_wint_and_fuse_bias(dev):
    ops = _ops()
    assert not ops.sf_head_fused_ok("f32", 8, 16, 64, 64, 13) and not ops.sf_head_fused_ok("bf16", 8, 16, 64, 64, 33)
    assert not ops.sf_head_fused_ok("bf16", 4, 16, 64, 64, 13) and not ops.sf_head_fused_ok("bf16", 8, 24, 64, 64, 13)
    assert not ops.sf_head_fused_ok("bf16", 8, 16, 32, 64, 13) and not ops.sf_head_fused_ok("bf16", 8, 16, 64, 96, 13)
    d = T.head_inputs((8, 16, 64, 1))
    b = {k: _to(d[k], "bf16", dev) for k in ("f0", "g1", "g2", "g3")}
    bad = torch.zeros(2, 4, 16, 64, dtype=torch.bfloat16, device=dev)
    assert ops.sf_head_fused(bad, _f32(d["w0"], dev), b["g1"], b["g2"], b["g3"], _f32(d["scale"], dev), _f32(d["shift2"], dev),
                             _f32(d["wc"], dev), _f32(d["bc"], dev), rc=True) == -2
    _same(ops.sf_head_wint(dev), T.wint_ref(), "sf_head_wint")
    g = T.gen(77)
    D = 96
    wf = torch.randn(D, 4 * D, generator=g, dtype=torch.float64)
    bs = [torch.randn(D, generator=g, dtype=torch.float64) for _ in range(4)]
    scale, shift = torch.randn(D, generator=g, dtype=torch.float64), torch.randn(D, generator=g, dtype=torch.float64)
    f = [t.float().double() for t in [wf] + bs + [scale, shift]]
    got = ops.sf_fuse_bias(*[_f32(t, dev) for t in f])
    ref = T.fuse_bias_ref(*f)
    err = float((_back(got) - ref).abs().max() / ref.abs().max())
    print(f"sf_fuse_bias rel err {err:.3e}")
    assert err <= 1e-6


# ================================================================================================ exact: dyadic resizes, pools
@pytest.mark.parametrize("dt", T.DTYPES)
def test_dyadic_resizes_are_exact(dev, dt):
    """inputs in multiples of 64: every weight a b / 4^(s+1), s <= 3, gives an integer"""
    ops = _ops()
    g = T.gen(21)
    for (B, h, w, C) in [(2, 1, 1, 8), (2, 2, 3, 16), (1, 5, 7, 32)]:                       # swin_bilinear_add x2
        x, y = 64 * T.randint(g, -2, 2, B, h, w, C), T.randint(g, -3, 3, B, 2 * h, 2 * w, C)
        yd = _to(y, dt, dev)
        ops.swin_bilinear_add_(yd, _to(x, dt, dev))
        _same(yd, y + T.bilinear_ref(x, 2 * h, 2 * w), f"swin_bilinear_add {h}x{w} x2 {dt}")
    for f in (2, 4, 8):                                                                    # sf_bilinear_nhwc into a channel slice
        B, h, w, C, ld = 2, 3, 5, 16, 40
        x = (256 if f == 8 else 64) * T.randint(g, -1, 1, B, h, w, C)
        out = torch.full((B, f * h, f * w, ld), 7.0, dtype=TDT[dt], device=dev)
        ops.sf_bilinear_nhwc(_to(x, dt, dev), f * h, f * w, out=out)
        ref = torch.full((B, f * h, f * w, ld), 7.0, dtype=torch.float64)
        ref[..., :C] = T.bilinear_ref(x, f * h, f * w)
        _same(out, ref, f"sf_bilinear_nhwc x{f} {dt}")
    if dt == "f32":                                                                        # the logits resize: both kernels
        for (h, w) in [(2, 3), (4, 1), (3, 5)]:
            H, W = 4 * h, 4 * w
            x = 64 * T.randint(g, -3, 3, 2, 3, h, w)
            fast = W % 4 == 0 and H % 8 == 0
            assert fast == ((h, w) != (3, 5))
            ref = T.bilinear_ref(x.permute(0, 2, 3, 1), H, W).permute(0, 3, 1, 2)
            _same(ops.sf_bilinear_nchw_f32(_f32(x, dev), H, W), ref, f"sf_bilinear_nchw_f32 {h}x{w} x4")
        x = 64 * T.randint(g, -3, 3, 1, 2, 3, 5)                                           # W % 4 != 0: the any-shape kernel
        _same(ops.sf_bilinear_nchw_f32(_f32(x, dev), 12, 10), T.bilinear_ref(x.permute(0, 2, 3, 1), 12, 10).permute(0, 3, 1, 2),
              "sf_bilinear_nchw_f32 any-shape")


@pytest.mark.parametrize("dt", T.DTYPES)
def test_power_of_two_pools_and_slices_are_exact(dev, dt):
    ops = _ops()
    g = T.gen(22)
    for n in (4, 2):
        for S in (1, 2, 3, 6):                      # S = 3, 6 on 2 x 2: more bins than pixels
            C, ld = 16, 24
            x = T.randint(g, -8, 8, 2, n, n, ld)
            _same(ops.swin_adaptive_avgpool(_to(x, dt, dev), C, S), T.avgpool_ref(x[..., :C], S), f"swin_adaptive_avgpool {n}->{S} {dt}")
    src = T.randint(g, -200, 200, 37, 40)
    _same(ops.sf_slice_cols(_f32(src, dev), 8, 16, dt), src[:, 8:24], f"sf_slice_cols {dt}")
    assert ops.sf_slice_cols(_f32(src, dev), 8, 12, "bf16", rc=True) == -2


@pytest.mark.parametrize("name", list(T.EW_LOOP))
def test_elementwise_kernels_loop_past_their_grid_cap(dev, name):
    """bf16, 1 048 576 chunks plus a remainder that is no multiple of 256: the grid-stride loop runs with a ragged last trip"""
    ops = _ops()
    c = T.EW_LOOP[name]
    g = T.gen(len(name))
    dt = "bf16"
    if name in ("swin_bilinear_add", "sf_bilinear_nhwc"):
        x = 64 * T.randint(g, -2, 2, c["B"], c["h"], c["w"], c["C"])
        H, W = 2 * c["h"], 2 * c["w"]
        up = T.bilinear_ref(x, H, W)
        if name == "swin_bilinear_add":
            y = T.randint(g, -3, 3, c["B"], H, W, c["C"])
            yd = _to(y, dt, dev)
            ops.swin_bilinear_add_(yd, _to(x, dt, dev))
            _same(yd, y + up, name)
        else:
            out = torch.full((c["B"], H, W, c["ld"]), 7.0, dtype=TDT[dt], device=dev)
            ops.sf_bilinear_nhwc(_to(x, dt, dev), H, W, out=out)
            got = _back(out)
            _same(got[..., :c["C"]], up, name)
            assert bool((got[..., c["C"]:] == 7).all())
    elif name == "swin_avgpool":
        x = T.randint(g, -8, 8, c["B"], c["h"], c["w"], c["C"])
        _same(ops.swin_adaptive_avgpool(_to(x, dt, dev), c["C"], c["S"]), T.avgpool_ref(x, c["S"]), name)
    elif name == "sf_upsample_sum_bn_relu":
        B, H, W, D = c["B"], c["H"], c["W"], c["D"]
        g0 = T.randint(g, -32, 32, B, H, W, D)
        g1, g2 = (-64 * T.randint(g, 0, 1, B, H >> i, W >> i, D) for i in (1, 2))
        g3 = 256 * T.randint(g, 0, 1, B, H >> 3, W >> 3, D)
        scale, shift2 = torch.ones(D, dtype=torch.float64), T.randint(g, -48, -32, D)
        ref = torch.relu(g0 + T.bilinear_ref(g1, H, W) + T.bilinear_ref(g2, H, W) + T.bilinear_ref(g3, H, W) + shift2)
        assert float(ref.max()) <= 256 and torch.equal(ref, ref.round())
        z = ops.sf_upsample_sum_bn_relu(_to(g0, dt, dev), _to(g1, dt, dev), _to(g2, dt, dev), _to(g3, dt, dev), _f32(scale, dev), _f32(shift2, dev))
        _same(z, ref, name)
    else:
        src = T.randint(g, -200, 200, c["rows"], c["ld"])
        _same(ops.sf_slice_cols(_f32(src, dev), c["col0"], c["ncols"], dt), src[:, c["col0"]:c["col0"] + c["ncols"]], name)


# ==================================================================================================== exact: the gather-form GEMM
@pytest.mark.parametrize("dt", T.DTYPES)
@pytest.mark.parametrize("case", T.GEMM_CASES, ids=lambda c: c[0])
def test_gemm_as_the_transformer_paths_use_it_is_exact(dev, case, dt):
    """ternary data: plain, into the first Cout columns of a 3 Cout-wide row (neighbours untouched) and with the in-place
    residual (ores is out)"""
    name, (N, H, W), Cin, Cout, R, stride, pad = case
    x, w, b = T.gemm_inputs(case)
    ref = F.conv2d(x, w, b, stride=stride, padding=pad).permute(0, 2, 3, 1)
    ops = _ops()
    xd, wd, bd = _to(x.permute(0, 2, 3, 1), dt, dev), _f32(w, dev), _f32(b, dev)
    _same(ops.conv2d_ex(xd, wd, bias=bd, stride=stride, pad=pad)["y"], ref, f"{name} {dt}")
    Ho, Wo = ref.shape[1:3]
    wide = torch.full((N, Ho, Wo, 3 * Cout), 5.0, dtype=TDT[dt], device=dev)
    ops.conv2d_ex(xd, wd, bias=bd, stride=stride, pad=pad, out=wide)
    got = _back(wide)
    _same(got[..., :Cout], ref, f"{name} {dt} out_ld")
    assert bool((got[..., Cout:] == 5).all()), "columns past Cout were written"
    res = T.randint(T.gen(5), -3, 3, N, Ho, Wo, Cout)
    assert float((ref + res).abs().max()) <= 256
    out = _to(res, dt, dev)
    ops.conv2d_ex(xd, wd, bias=bd, stride=stride, pad=pad, out=out, ores=out)
    _same(out, ref + res, f"{name} {dt} in-place residual")


# ======================================================================================= derived bound: exact pre-activation + GELU
@pytest.mark.parametrize("dt", T.DTYPES)
@pytest.mark.parametrize("case", T.DW_CASES, ids=lambda c: c[0])
def test_dwconv3x3_gelu_error_is_the_gelus_alone(dev, case, dt):
    """integer inputs, weights and bias: the convolution is exact in either dtype, so the error is the GELU's (T.gelu_bound derives
    the bound); a wrong, missing or doubled tap changes the pre-activation by an integer"""
    name, B, H, W, C, lmax, _ = case
    x, w, b = T.dw_inputs(case)
    pre, ref = T.dwconv_gelu_ref(x, w, b)
    with _tuned(FLAIR_SF_DW_L=lmax):
        y = _ops().sf_dwconv3x3_gelu(_to(x, dt, dev), _f32(w, dev), _f32(b, dev))
    _within(y, ref, T.gelu_bound(dt, pre, ref), f"sf_dwconv3x3_gelu {name} {dt}")


def test_dwconv_default_segment_length_follows_the_dtype_at_every_call(dev):
    """an fp32 launch first must not fix the bf16 default (both results stay right whatever the order; FLAIR_SF_DW_L = 0 restores
    the per-dtype default after a pinned value)"""
    case = T.DW_CASES[0]
    x, w, b = T.dw_inputs(case)
    pre, ref = T.dwconv_gelu_ref(x, w, b)
    ops = _ops()
    with _tuned(FLAIR_SF_DW_L=16):
        ops.sf_dwconv3x3_gelu(_to(x, "f32", dev), _f32(w, dev), _f32(b, dev))
    for dt in ("f32", "bf16", "f32"):
        y = ops.sf_dwconv3x3_gelu(_to(x, dt, dev), _f32(w, dev), _f32(b, dev))
        _within(y, ref, T.gelu_bound(dt, pre, ref), f"sf_dwconv3x3_gelu default after pinned, {dt}")
    assert ops.sf_dwconv3x3_gelu(_to(x[..., :2].repeat(1, 1, 1, 3), "f32", dev), _f32(w, dev), _f32(b, dev), rc=True) == -2


@pytest.mark.parametrize("dt", T.DTYPES)
def test_gemm_gelu_epilogue(dev, dt):
    """ogelu: fp32 0.5 v (1 + erff(v / sqrt 2)) of the accumulator + bias; in bf16 of the ALREADY ROUNDED tile (chunk_to_f on the
    stored chunk, conv_igemm.hip), exact here because the pre-activation is a small integer, then one more rounding: half a bf16
    ulp on top of the fp32 bound.  -6 where the epilogue does not exist."""
    from flair_amd._lib import FlairHipError
    ops = _ops()
    for (N, H, W, Cin, Cout) in [(1, 7, 7, 96, 384), (2, 5, 13, 96, 384)]:
        g = T.gen(N + Cout)
        x = T.randint(g, -1, 1, N, Cin, H, W)
        w = T.randint(g, -1, 1, Cout, Cin, 1, 1) * (torch.rand(Cout, Cin, 1, 1, generator=g) < 0.2).double()
        b = T.randint(g, -2, 2, Cout)
        pre = F.conv2d(x, w, b).permute(0, 2, 3, 1)
        assert float(pre.abs().max()) <= 256 and float(pre.abs().max()) >= 6
        ref = T.gelu_ref(pre)
        xd = _to(x.permute(0, 2, 3, 1), dt, dev)
        y = ops.conv2d_ex(xd, _f32(w, dev), bias=_f32(b, dev), pad=0, ogelu=True)["y"]
        bound = T.gelu_bound("f32", pre, ref) * (1 if dt == "f32" else 2) + (0.5 * T.ulp(ref, 7) if dt == "bf16" else 0)
        _within(y, ref, bound, f"gemm + gelu {N}x{H}x{W} {dt}")
        for kw in (dict(want_nchw=True), dict(in_scale=torch.ones(Cin, device=dev), in_shift=torch.zeros(Cin, device=dev))):
            with pytest.raises(FlairHipError, match="code -6"):
                ops.conv2d_ex(xd, _f32(w, dev), bias=_f32(b, dev), pad=0, ogelu=True, **kw)


# ============================================================================== derived bound: non-dyadic resizes and pools
def _resize_bound(dt, n_in, M, ref):
    """fp32: the source coordinate is fl(fl((dst + 0.5) * fl(in / out)) - 0.5): three roundings on a value <= in, |ds| <= 3 u in per
    axis, and the blend is bilinear with slope <= 2 M in each coordinate: 12 u in M; the blend itself is four (1 - l) / l
    products, three additions and two more products on values <= M: 10 u M.  bf16 adds one output ulp."""
    b = torch.full_like(ref, (12 * n_in + 10) * U * M)
    return b + (T.ulp(ref, 7) if dt == "bf16" else 0)


@pytest.mark.parametrize("dt", T.DTYPES)
def test_nondyadic_resizes_and_pools(dev, dt):
    ops = _ops()
    g = T.gen(31)
    for n in (1, 2, 3, 6):                                  # the pyramid-pooling upsamples (6 -> 4 is a downsample)
        for out_n in (4, 16):
            x = T.rnd(torch.randn(2, n, n, 16, generator=g, dtype=torch.float64), dt)
            ref = T.bilinear_ref(x, out_n, out_n)
            got = ops.sf_bilinear_nhwc(_to(x, dt, dev), out_n, out_n)
            _within(got, ref, _resize_bound(dt, n, float(x.abs().max()), ref), f"sf_bilinear_nhwc {n}->{out_n} {dt}")
    for (h, w, H, W) in [(5, 7, 8, 9), (3, 3, 7, 5)]:        # swin_bilinear_add at a non-integer ratio
        x = T.rnd(torch.randn(2, h, w, 16, generator=g, dtype=torch.float64), dt)
        y = T.rnd(torch.randn(2, H, W, 16, generator=g, dtype=torch.float64), dt)
        ref = y + T.bilinear_ref(x, H, W)
        yd = _to(y, dt, dev)
        ops.swin_bilinear_add_(yd, _to(x, dt, dev))
        M = float(x.abs().max() + y.abs().max())
        _within(yd, ref, _resize_bound(dt, max(h, w), M, ref), f"swin_bilinear_add {h}x{w}->{H}x{W} {dt}")
    for n in (7, 16):                                       # sums of up to n^2 terms: (count + 2) u M after the division
        for S in (1, 2, 3, 6):
            x = T.rnd(torch.randn(2, n, n, 24, generator=g, dtype=torch.float64), dt)
            ref = T.avgpool_ref(x[..., :16], S)
            count = max(T.pool_bins(n, S)) ** 2
            bound = torch.full_like(ref, (count + 2) * U * float(x.abs().max())) + (T.ulp(ref, 7) if dt == "bf16" else 0)
            _within(ops.swin_adaptive_avgpool(_to(x, dt, dev), 16, S), ref, bound, f"swin_adaptive_avgpool {n}->{S} {dt}")


# ================================================================================================ measured bound: LayerNorms
def _ln_params(C, g):
    return (1 + 0.5 * torch.randn(C, generator=g, dtype=torch.float64)).float().double(), torch.randn(C, generator=g, dtype=torch.float64).float().double()


@pytest.mark.parametrize("dt", T.DTYPES)
@pytest.mark.parametrize("C", T.SF_LN_C)
def test_sf_layernorm(dev, C, dt):
    ops = _ops()
    g = T.gen(C)
    gam, bet = _ln_params(C, g)
    for kind in T.LN_KINDS:
        x, eps = T.ln_rows(kind, 37, C, g)                  # 37 rows: the last workgroup is partly dead
        x = T.rnd(x, dt)
        y = ops.sf_layernorm(_to(x, dt, dev), _f32(gam, dev), _f32(bet, dev), eps)
        _measured("sf_layernorm", dt, f"C{C}_{kind}", y, T.layernorm_ref(x, gam, bet, eps))


@pytest.mark.parametrize("dt", T.DTYPES)
def test_sf_layernorm_refuses_more_than_two_chunks_per_lane(dev, dt):
    C = 516 if dt == "f32" else 1032
    assert T.sf_ln_group(dt, C) is None
    x = torch.zeros(4, C, dtype=TDT[dt], device=dev)
    p = torch.ones(C, device=dev)
    assert _ops().sf_layernorm(x, p, p, 1e-5, rc=True) == -2


@pytest.mark.parametrize("dt", T.DTYPES)
@pytest.mark.parametrize("C", T.SWIN_LN_C)
def test_swin_layernorm(dev, C, dt):
    ops = _ops()
    g = T.gen(C + 1)
    gam, bet = _ln_params(C, g)
    for kind in T.LN_KINDS:
        x, eps = T.ln_rows(kind, 37, C, g)
        x = T.rnd(x, dt)
        out = torch.full((37, C + 32), 3.0, dtype=TDT[dt], device=dev)      # ld > C: the columns past C stay
        ops.swin_layernorm(_to(x, dt, dev), _f32(gam, dev), _f32(bet, dev), eps, out=out)
        _measured("swin_layernorm", dt, f"C{C}_{kind}", out[:, :C], T.layernorm_ref(x, gam, bet, eps))
        assert bool((out[:, C:] == 3).all())


@pytest.mark.parametrize("dt", T.DTYPES)
@pytest.mark.parametrize("C", T.MERGE_C)
def test_swin_patch_merge_ln(dev, C, dt):
    ops = _ops()
    g = T.gen(C + 2)
    gam, bet = _ln_params(4 * C, g)
    if T.swin_ln_group(dt, 4 * C) is None:                  # fp32 rows of 3072: twelve chunks per lane, refused
        x = torch.zeros(1, 2, 2, C, dtype=TDT[dt], device=dev)
        assert ops.swin_patch_merge_ln(x, _f32(gam, dev), _f32(bet, dev), 1e-5, rc=True) == -2
        return
    for (H, W) in T.MERGE_GRIDS:
        for eps in (1e-5, 1e-6):
            x = 0.3 * torch.randn(2, H, W, C, generator=g, dtype=torch.float64)
            for qd, (r, c) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):   # every quadrant its own constant
                x[:, r::2, c::2] += (-1.0, 0.5, 2.0, -2.5)[qd]
            x = T.rnd(x, dt)
            y = ops.swin_patch_merge_ln(_to(x, dt, dev), _f32(gam, dev), _f32(bet, dev), eps)
            _measured("swin_patch_merge_ln", dt, f"C{C}_{H}x{W}_eps{eps:g}", y, T.patch_merge_ref(x, gam, bet, eps))
    assert ops.swin_patch_merge_ln(torch.zeros(1, 3, 2, C, dtype=TDT[dt], device=dev), _f32(gam, dev), _f32(bet, dev), 1e-5, rc=True) == -2


# ========================================================================================= measured bound: attention, real softmax
@pytest.mark.parametrize("dt", T.DTYPES)
@pytest.mark.parametrize("case", T.SWIN_GATHER_CASES, ids=lambda c: c[0])
def test_swin_attention_random(dev, case, dt):
    """table and biases from N(0, 1), not the library's 0.02: an index error in the table or a wrong region label is an O(1)
    error; the pad tokens take part as keys and values with the bias values"""
    name, B, H, W, heads, shift = case
    g = T.gen(500 + sum(map(ord, name)))
    C = 32 * heads
    qkv = T.rnd(torch.randn(B, H, W, 3 * C, generator=g, dtype=torch.float64), dt)
    bias = torch.randn(3 * C, generator=g, dtype=torch.float64).float().double()
    table = torch.randn(169, heads, generator=g, dtype=torch.float64).float().double()
    out = _ops().swin_window_attention(_to(qkv, dt, dev), _f32(bias, dev), _f32(table, dev), heads, shift)
    # the kernel rounds the pad tokens' k and v to the compute dtype when it stores them to LDS; so does the reference
    ref = T.window_attention_ref(qkv, torch.cat([bias[:C], T.rnd(bias[C:], dt)]), table, heads, shift, round_p=dt == "bf16")
    _measured("swin_window_attention", dt, name, out, ref)


@pytest.mark.parametrize("mode", ["f32", "bf16", "bf16_one_tile"])
@pytest.mark.parametrize("Nk", [16, 144, 256])
def test_sf_attention_random(dev, Nk, mode):
    dt = mode[:4].rstrip("_")
    g = T.gen(Nk)
    B, heads, N = 2, 2, 200
    hid = 64 * heads
    q = T.rnd(torch.randn(B, N, hid, generator=g, dtype=torch.float64), dt)
    kv = T.rnd(torch.randn(B, Nk, 2 * hid, generator=g, dtype=torch.float64), dt)
    kvd = _to(kv, dt, dev)
    with _tuned(FLAIR_SF_ATT2=0 if mode.endswith("one_tile") else 1):
        out = _ops().sf_attention(_to(q, dt, dev), kvd[..., :hid], kvd[..., hid:], kv_ld=2 * hid)
    ref = T.sf_attention_ref(q, kv[..., :hid], kv[..., hid:], round_p=dt == "bf16")
    _measured("sf_attention_one_tile" if mode.endswith("one_tile") else "sf_attention", dt, f"Nk{Nk}", out, ref)


@pytest.mark.parametrize("att2", [1, 0], ids=["two_tile", "one_tile"])
def test_sf_attention_denominator_is_from_the_unrounded_p(dev, att2):
    """derived bound (T.denominator_inputs): the bf16 kernels round P for the second product but sum the unrounded values; with
    every P 0.30 % above its unrounded value the output is 0.29 % above V, and half a bf16 ulp there is 0.20 %"""
    q, kv, want, _ = T.denominator_inputs()
    hid = q.shape[-1]
    kvd = _to(kv, "bf16", dev)
    with _tuned(FLAIR_SF_ATT2=att2):
        out = _ops().sf_attention(_to(q, "bf16", dev), kvd[..., :hid], kvd[..., hid:], kv_ld=2 * hid)
    _within(out, want, T.denominator_bound(want), f"sf_attention denominator att2={att2}")


def test_sf_attention_refusals(dev):
    ops = _ops()
    q = torch.zeros(1, 16, 64, dtype=torch.bfloat16, device=dev)
    for Nk, hid in ((24, 64), (272, 64)):
        kv = torch.zeros(1, Nk, hid, dtype=torch.bfloat16, device=dev)
        assert ops.sf_attention(q, kv, kv, rc=True) == -2
    assert ops.sf_attention(torch.zeros(1, 16, 96, dtype=torch.bfloat16, device=dev), torch.zeros(1, 16, 96, dtype=torch.bfloat16, device=dev),
                            torch.zeros(1, 16, 96, dtype=torch.bfloat16, device=dev), rc=True) == -2


# ================================================================================================ measured bound: fused Mix-FFN
def _ffn_params(C, g):
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
    p = dict(ln_g=1 + 0.2 * r(C), ln_b=0.2 * r(C), w1=T.bf16r(r(4 * C, C) / C ** 0.5), b1=0.2 * r(4 * C), dw_w=r(4 * C, 3, 3) / 3,
             dw_b=0.2 * r(4 * C), w2=T.bf16r(r(C, 4 * C) / (4 * C) ** 0.5), b2=0.2 * r(C))
    return {k: v.float().double() for k, v in p.items()}


@pytest.mark.parametrize("with_ln", [False, True], ids=["plain", "out_ln"])
@pytest.mark.parametrize("grid", [(8, 8), (16, 24), (8, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", [64, 128])
def test_ffn_fused_against_the_rounding_faithful_restatement(dev, C, grid, with_ln):
    """8 x 8: one tile, its whole halo outside the image; 16 x 24 and 8 x 16: interior halos read the neighbouring tiles"""
    ops = _ops()
    H, W = grid
    g = T.gen(C + H + W)
    p = _ffn_params(C, g)
    x = T.bf16r(torch.randn(2, H, W, C, generator=g, dtype=torch.float64))
    ln2 = _ln_params(C, g) if with_ln else None
    eps = 1e-6
    assert ops.sf_ffn_fused_ok("bf16", C, H, W)
    d = {k: _f32(v, dev) for k, v in p.items()}
    out, out_ln = ops.sf_ffn_fused(_to(x, "bf16", dev), d["ln_g"], d["ln_b"], d["w1"], d["b1"], d["dw_w"], d["dw_b"], d["w2"], d["b2"], eps,
                                   ln2_g=_f32(ln2[0], dev) if ln2 else None, ln2_b=_f32(ln2[1], dev) if ln2 else None, want_ln=with_ln)
    ref, ref_ln = T.mix_ffn_ref(x, p, eps, faithful=True, ln2=ln2)
    _measured("sf_ffn_fused", "bf16", f"C{C}_{H}x{W}{'_ln' if with_ln else ''}", out, ref)
    if with_ln:
        _measured("sf_ffn_fused_ln", "bf16", f"C{C}_{H}x{W}", out_ln, ref_ln)


def test_ffn_fused_refusals(dev):
    ops = _ops()
    assert not ops.sf_ffn_fused_ok("f32", 64, 8, 8) and not ops.sf_ffn_fused_ok("bf16", 320, 8, 8)
    assert not ops.sf_ffn_fused_ok("bf16", 64, 12, 8) and not ops.sf_ffn_fused_ok("bf16", 64, 8, 4)
    C = 64
    p = {k: _f32(v, dev) for k, v in _ffn_params(C, T.gen(1)).items()}
    x = torch.zeros(1, 8, 8, C, dtype=torch.bfloat16, device=dev)
    other = torch.zeros_like(x)
    args = (p["ln_g"], p["ln_b"], p["w1"], p["b1"], p["dw_w"], p["dw_b"], p["w2"], p["b2"], 1e-6)
    assert ops.sf_ffn_fused(x, *args, out=x, rc=True) == -2                                                     # x == out
    assert ops.sf_ffn_fused(x, *args, ln2_g=p["ln_g"], ln2_b=p["ln_b"], out=other, out_ln=x, rc=True) == -2     # out_ln == x
    assert ops.sf_ffn_fused(x, *args, out=other, out_ln=torch.zeros_like(x), rc=True) == -2                     # out_ln without its norm
    assert ops.sf_ffn_fused(torch.zeros(1, 8, 12, C, dtype=torch.bfloat16, device=dev), *args, rc=True) == -2
