"""Exact operator tests of the fused backward forms of the U-Net training step: what csrc/unet.hip launches on the backward path,
one kernel at a time, on small-integer data against fp64 CPU references with torch.equal (tests/bwd_fused_cases.py holds the
cases and asserts, on the references alone, that they are inside the exact range).

Every output and every partial-sum buffer is pre-filled with NaN (sums) or a sentinel (tensors) before the call: an element a
kernel never writes fails the comparison.  The convolution, fused stem weight-gradient, bn_backward, plain and accumulating
max-pool backward, bn_act_maxpool, upcat_bwd and pack_weights_all launches assert through the launch profile which kernels ran,
and that each ran once; the max-pool backward with the fused reduction, bn_act, ew_add, colsum, pack_weight and the unfused stem
route do not (ew_add and colsum record no profile entry).

Argument -> cases (every argument unet.hip sets on the backward path):
  ConvArgs  bnr_y / bnr_scale / bnr_shift / bnr_partial / bnr_C   test_bnr_epilogue_exact (all), test_bnr_chain_into_bn_backward
            bnr_out                                               bnr_out_acc_hg64to64, bnr_out_acc_mask_hg128to128
            bnr_mask                                              bnr_mask_*, bnr_out_acc_mask_*, bnr_pool_mask_*
            accumulate (+ bnr)                                    bnr_out_acc_*, bnr_pool_acc_hg64to128_c128
            acc_src (+ bnr)                                       bnr_mask_accsrc_hg128to128
            pool_c0 / out_skip / skip_accumulate (+ bnr)          bnr_pool_*
            out_sub, ncls, cls_w, cls_kpad                        test_parity_dgrad_exact (R = 3 cases)
            out_sub alone + accumulate (1x1 / stride 2)           par_1x1_64to128_accumulate / _write
            src0, C0, N, H*, W*, R, S, out_mul, pad, in_div, Cout, Kg, Kpad, w, out, out_ld
                                                                  every case here and in test_gpu_ops_exact.py
  WgradArgs fuse_y / fuse_coef / fuse_msc / fuse_msh              test_stem_wgrad_fused_apply_*
            (x0, x1, up0, dy, dy_ld, in_scale, cus, dbias: test_gpu_ops_exact.py)
  bn_backward out / mscale, mshift / neither                      bn_mask_out_*, bn_mask_mscale_*, bn_no_relu_*
            accumulate_param                                      bn_accumulate_param_c64 (the network passes 0; the argument exists)
            dres, dres_accumulate                                 bn_dres_*, bn_premasked_nblk640_c16, bn_rows16384_out_c64
            dy == nullptr (coefficients for the stem)             bn_coefficients_only_c16, test_stem_wgrad_fused_apply_matches_the_separate_pass
            partial + pre_nblk, premasked                         bn_pre_nblk*, bn_premasked_*, test_bnr_chain_into_bn_backward
  maxpool3x3s2_bwd accumulate, bnr_y / bnr_msc / bnr_msh / bnr_partial      test_maxpool_backward_accumulate_and_fused_reduction
  bn_act_maxpool3x3s2, upcat_bwd, ew_add, colsum, pack_weights_all          the tests named after them
  pack_weight (the packer of flair_conv2d_forward / _backward / _ex)        test_pack_weights_all_against_the_layout_formula
Not covered here:
  ConvArgs::xcd_remap is set by the launcher (FLAIR_XCD_REMAP), dbg by diagnostic builds only.
  The 128-wide halo-GEMM's 16x16 and 32x8 tile instantiations with the fused reduction: under the default switches launch_hg_t
  gives every Cout % 128 == 0 layer 128-pixel (16x8) tiles, so those two are reachable only with FLAIR_HG_DMA=0 and
  FLAIR_HG_VARIANT=0, and the library reads the latter once per process; the 128-wide BNR cases here all run on 16x8 tiles.
  launch_conv's "ncls without out_sub" refusal cannot be reached through flair_conv2d_ex; mode 2 with another geometry is (-6).

Both dtypes of a case share one reference (the case modules cache the last two), so the dtype parameter varies fastest.  One
process, well under 1 GB of device memory; the 120 tests of this file take 7 s on an MI355X (the slowest 0.7 s)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bwd_fused_cases as B
import exact_cases as E
import launch_helpers as LH

pytestmark = pytest.mark.gpu

TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
SENTINEL = 99.0     # pre-fill of output tensors: an element left at it differs from its expectation
NAN = float("nan")


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def _nhwc(x, dt, dev):
    return None if x is None else x.permute(0, 2, 3, 1).contiguous().to(device=dev, dtype=TDT[dt])


def _nchw(y):
    return y.float().cpu().permute(0, 3, 1, 2).double()


def _rows(t, dt, dev):
    return None if t is None else t.contiguous().to(device=dev, dtype=TDT[dt])


def _same(got, ref, what):
    """torch.equal with a message that says where (NaN never equals anything: an unwritten element fails)."""
    got, ref = got.double().cpu(), ref.double()
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {ref.numel()} elements differ, first at {i}: got {float(got[i])}, "
                             f"expected {float(ref[i])}; last at {tuple(int(v) for v in bad[-1])}")


_tuned = functools.partial(LH.tuned, defaults=E.TUNE_DEFAULTS)
# the convolution, weight-gradient, BatchNorm-backward, pooling, upcat and pack launches
_profiled = functools.partial(LH.profiled, keep=("conv", "wgrad", "bn_bwd_", "bn_act", "maxpool_", "upcat_bwd", "pack_weights_all"))


def _backed(t, dt, dev, numel):
    """NHWC copy of t at the start of a zero-filled allocation of `numel` elements (the mask sources of the pooled cases: a kernel
    that wrongly indexed them with the full-resolution geometry would still read memory this test owns)."""
    v = _nhwc(t, dt, dev)
    buf = torch.zeros(max(numel, v.numel()), dtype=TDT[dt], device=dev)
    buf[:v.numel()] = v.flatten()
    return buf[:v.numel()].view(v.shape)


# ------------------------------------------------------------------------------------------------ a. BNR epilogue of the data gradient
def _run_bnr(dev, dt, c):
    """One flair_conv2d_ex launch of a BNR case with every check of (a); returns what the chain test feeds on."""
    from flair_amd import ops
    r = B.bnr_reference(c)
    B.check_bnr_range(c, r)
    B.check_bnr_dispatch_and_loops(c)
    x0, w = _nhwc(r["x0"], dt, dev), r["w"].to(dev)
    full = c.N * c.H * c.W * c.Cout
    y = _backed(r["y"], dt, dev, full)
    bout = _backed(r["out"], dt, dev, full) if c.from_out else None
    scale, shift = r["scale"].to(dev), r["shift"].to(dev)
    shape = (c.N, c.H // 2, c.W // 2, c.pool_c0) if c.pool_c0 else (c.N, c.H, c.W, c.Cout)
    src = None
    if c.accumulate and not c.acc_src:
        out = _nhwc(r["prev"], dt, dev)
    else:
        out = torch.full(shape, SENTINEL, dtype=TDT[dt], device=dev)
        src = _nhwc(r["prev"], dt, dev) if c.acc_src else None
    skip = None
    if c.pool_c0 and c.pool_c0 < c.Cout:
        skip = (_nhwc(r["prev_skip"], dt, dev) if c.skip_accumulate else
                torch.full((c.N, c.H, c.W, c.Cout - c.pool_c0), SENTINEL, dtype=TDT[dt], device=dev))
    kw = dict(mode=1, out=out, accumulate=c.accumulate, acc_src=src, pool_c0=c.pool_c0, out_skip=skip, skip_accumulate=c.skip_accumulate,
              bnr_y=y, bnr_out=bout, bnr_scale=scale, bnr_shift=shift, bnr_mask=c.bnr_mask)
    with _tuned(c.tune):
        rows = ops.conv2d_ex_grid_rows(x0, w, **kw)
        want_rows = c.grid_rows(dt)
        assert want_rows is None or rows == want_rows, (c.name, dt, "row blocks", rows, want_rows)
        partial = torch.full((2, c.Cy, rows), NAN, dtype=torch.float32, device=dev)
        _, ran = _profiled(lambda: ops.conv2d_ex(x0, w, bnr_partial=partial, **kw))
    assert ran == {c.launch(dt)[1]: 1}, (c.name, dt, ran)
    _same(_nchw(out), r["stored"], "the stored gradient (dz m with bnr_mask, else dz)")
    if skip is not None:
        _same(_nchw(skip), r["skip"], "skip columns (never masked, whatever bnr_mask says)")
    assert not bool(torch.isnan(partial).any()), (c.name, dt, "partial rows never written:", int(torch.isnan(partial).sum()))
    _same(partial.double().sum(2), torch.stack([r["s1"], r["s2"]]), "sum over the row blocks of (sum dz m, sum dz m y)")
    _same(_nchw(y), r["y"], "bnr_y is left alone")
    if src is not None:
        _same(_nchw(src), r["prev"], "acc_src is left alone")
    return {"r": r, "stored": out, "partial": partial, "rows": rows, "y": y, "out": bout, "scale": scale, "shift": shift}


@pytest.mark.parametrize("dt", E.DTYPES)
@pytest.mark.parametrize("case", B.BNR_CASES, ids=lambda c: c.name)
def test_bnr_epilogue_exact(dev, dt, case):
    _run_bnr(dev, dt, case)


def test_bnr_refusals(dev):
    """launch_conv's own -6 comes back unchanged; a partial with too few rows is -100 before anything is launched."""
    from flair_amd import ops
    from flair_amd._lib import FlairHipError
    g = torch.Generator().manual_seed(1)
    vec = lambda n: torch.ones(n, device=dev)

    def setup(Cc, H, W):
        x = _nhwc(E.ternary((1, Cc, H, W), g, 0.5), "f32", dev)
        return x, E.ternary((Cc, Cc, 3, 3), g, 0.5).to(dev), torch.zeros_like(x), torch.full((2, Cc, 64), NAN, device=dev)

    x, w, y, part = setup(64, 10, 12)                                      # gather-form shape
    with pytest.raises(FlairHipError, match=r"code -6"):
        ops.conv2d_ex(x, w, mode=1, bnr_y=y, bnr_scale=vec(64), bnr_shift=vec(64), bnr_partial=part)
    assert bool(torch.isnan(part).all())
    x, w, y, part = setup(64, 24, 96)                                      # halo-GEMM shape
    with pytest.raises(FlairHipError, match=r"code -6"):                   # masked store without the reduction
        ops.conv2d_ex(x, w, mode=1, bnr_mask=True)
    with pytest.raises(FlairHipError, match=r"code -6"):                   # lazy input together with the reduction
        ops.conv2d_ex(x, w, mode=1, in_scale=vec(64), in_shift=vec(64), bnr_y=y, bnr_scale=vec(64), bnr_shift=vec(64), bnr_partial=part)
    assert ops.conv2d_ex_grid_rows(x, w, mode=1, bnr_y=y, bnr_scale=vec(64), bnr_shift=vec(64)) == 9
    part8 = torch.full((2, 64, 8), NAN, device=dev)
    with pytest.raises(FlairHipError, match=r"code -100"):                 # 9 row blocks, room for 8
        ops.conv2d_ex(x, w, mode=1, bnr_y=y, bnr_scale=vec(64), bnr_shift=vec(64), bnr_partial=part8)
    assert bool(torch.isnan(part8).all()) and bool(torch.isnan(part).all())
    x, w, y, part = setup(16, 16, 64)                                      # persistent small-channel kernel
    with pytest.raises(FlairHipError, match=r"code -6"):
        ops.conv2d_ex(x, w, mode=1, bnr_y=y, bnr_scale=vec(16), bnr_shift=vec(16), bnr_partial=part, bnr_mask=True)
    with pytest.raises(FlairHipError, match=r"code -6"):
        ops.conv2d_ex(x, w, mode=1, bnr_y=y, bnr_out=y, bnr_scale=vec(16), bnr_shift=vec(16), bnr_partial=part)
    assert bool(torch.isnan(part).all())


# ------------------------------------------------------------------------------------------------ b. bn_backward
def _check_bn(dt, got, ref, c_dres, want_dy, exact_dy=True):
    _same(got["dgamma"], ref["dgamma"], "dgamma")
    _same(got["dbeta"], ref["dbeta"], "dbeta")
    if exact_dy:
        _same(got["coef"], ref["coef"], "k1 | k2 | k3")
    if want_dy:
        if exact_dy:
            _same(got["dy"], B.round_once(ref["dy"], dt), "dy (the fp64 reference rounded once)")
        else:
            err = _rel(got["dy"].cpu(), ref["dy"])
            print(f"dy relative error {err:.3e} (bound {B.TOL[dt]})")
            assert err < B.TOL[dt], err
    if c_dres:
        _same(got["dres"], ref["dres"], "dres")


@pytest.mark.parametrize("dt", E.DTYPES)
@pytest.mark.parametrize("case", B.BN_CASES, ids=lambda c: c.name)
def test_bn_backward_ex_exact(dev, dt, case):
    from flair_amd import ops
    c, r = case, B.bn_reference(case)
    f = lambda k: None if r.get(k) is None else r[k].to(dev)
    y = _rows(r["y"], dt, dev)
    kw = dict(gamma=f("gamma"))
    if c.mask == "out":
        kw["out"] = _rows(r["out"], dt, dev)
    elif c.mask == "mscale":
        kw.update(mscale=f("scale"), mshift=f("shift"))
    if c.pre_nblk:
        kw.update(partial=r["partial"].float().contiguous().to(dev), pre_nblk=c.pre_nblk, premasked=c.mask == "premasked")
    if c.accumulate_param:
        kw.update(dgamma=f("prev_dgamma").clone(), dbeta=f("prev_dbeta").clone(), accumulate_param=True)
    else:
        kw.update(dgamma=torch.full((c.C,), NAN, device=dev), dbeta=torch.full((c.C,), NAN, device=dev))
    if c.dres:
        kw.update(dres=_rows(r["prev_dres"], dt, dev) if c.dres == "accumulate" else torch.full_like(y, SENTINEL),
                  dres_accumulate=c.dres == "accumulate")
    kw.update(dy=torch.full_like(y, NAN) if c.want_dy else None, want_dy=c.want_dy, coef=torch.full((3, c.C), NAN, device=dev))
    got, ran = _profiled(lambda: ops.bn_backward_ex(_rows(r["dout"], dt, dev), y, f("mean"), f("invstd"), **kw))
    want = {"bn_bwd_finalize": 1}
    if not c.pre_nblk:
        want["bn_bwd_reduce"] = 1
    if c.want_dy:
        want["bn_bwd_apply"] = 1
    assert ran == want, (c.name, dt, ran)
    _check_bn(dt, got, r, c.dres, c.want_dy)
    assert got["dy"] is None or c.want_dy


def test_bn_backward_ex_refusals(dev):
    from flair_amd import ops
    z = torch.zeros(256, 16, device=dev)
    v = torch.ones(16, device=dev)
    part = torch.zeros(2, 16, 4, device=dev)
    assert ops.bn_backward_ex(z, z, v, v, premasked=True, rc=True) == -2                       # premasked needs the producer's partial
    assert ops.bn_backward_ex(z, z, v, v, partial=part, pre_nblk=4, rc=True) == -2             # producer-side sums need a mask source
    wide = torch.zeros(8, 1032, device=dev, dtype=torch.bfloat16)                              # 129 chunk columns
    v2 = torch.ones(1032, device=dev)
    assert ops.bn_backward_ex(wide, wide, v2, v2, rc=True) == -2
    assert ops.bn_backward_ex(z, z, v, v, want_dy=False, want_dres=True, rc=True) == -1        # the apply pass always writes dy


# ------------------------------------------------------------------------------------------------ c. the chain the network runs
@pytest.mark.parametrize("dt", E.DTYPES)
@pytest.mark.parametrize("name,how", B.CHAIN_CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_bnr_chain_into_bn_backward(dev, dt, name, how):
    """The [2][C][nblk] layout contract between the two kernels: the data gradient's stored gradient and partial go straight into
    bn_backward (pre_nblk = the launch's row blocks); reference: data gradient -> mask -> BatchNorm backward, all fp64.
    dz, dgamma, dbeta are exact; dy is exact where the row count is a power of two and within TOL elsewhere."""
    from flair_amd import ops
    c = B.BNR_BY_NAME[name]
    a = _run_bnr(dev, dt, c)
    b = B.chain_reference(name)
    Cy = c.Cy
    flat = lambda t: t.reshape(-1, Cy)
    kw = dict(gamma=b["gamma"].to(dev), partial=a["partial"], pre_nblk=a["rows"])
    if how == "premasked":
        kw["premasked"] = True
    elif how == "out":
        kw["out"] = flat(a["out"])
    else:
        kw.update(mscale=a["scale"], mshift=a["shift"])
    kw.update(dy=torch.full_like(flat(a["y"]), NAN), dgamma=torch.full((Cy,), NAN, device=dev), dbeta=torch.full((Cy,), NAN, device=dev))
    got, ran = _profiled(lambda: ops.bn_backward_ex(flat(a["stored"]), flat(a["y"]), b["mean"].to(dev), b["invstd"].to(dev), **kw))
    assert ran == {"bn_bwd_finalize": 1, "bn_bwd_apply": 1}, (name, dt, ran)
    _check_bn(dt, got, b, "", True, exact_dy=b["pow2"])


# ------------------------------------------------------------------------------------------------ d. parity-class stride-2 data gradient
@pytest.mark.parametrize("dt", E.DTYPES)
@pytest.mark.parametrize("case", B.PARITY_CASES, ids=lambda c: c.name)
def test_parity_dgrad_exact(dev, dt, case):
    from flair_amd import ops
    c, r = case, B.parity_reference(case)
    B.check_parity_case(c, r)
    prev = r["prev"] if c.accumulate else torch.full_like(r["prev"], SENTINEL)
    dx = _nhwc(prev, dt, dev)
    _, ran = _profiled(lambda: ops.conv2d_ex(_nhwc(r["dy"], dt, dev), r["w"].to(dev), mode=2, stride=2, pad=c.pad, out=dx, accumulate=c.accumulate))
    assert ran == {c.launch(dt)[1]: 1, "pack_weights_all": 1}, (c.name, dt, ran)
    want = r["dx"] if c.accumulate else torch.where(r["touched"], r["grad"], prev.double())
    _same(_nchw(dx), want, "dx (pixels a 1x1 layer does not reach keep what was there)")


def test_parity_dgrad_refusals(dev):
    from flair_amd import ops
    from flair_amd._lib import FlairHipError
    g = torch.Generator().manual_seed(2)
    dy = _nhwc(E.ternary((1, 64, 5, 7), g, 0.5), "f32", dev)
    w = E.ternary((64, 64, 3, 3), g, 0.5).to(dev)
    dx = torch.full((1, 10, 14, 64), SENTINEL, device=dev)
    for kw in (dict(stride=1, pad=1), dict(stride=2, pad=0)):
        with pytest.raises(FlairHipError, match=r"code -6"):
            ops.conv2d_ex(dy, w, mode=2, out=dx, **kw)
    assert bool((dx == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ e. pack_weights_all
def _pack_bytes(dst, dt):
    if dt == "f32":
        return np.ascontiguousarray(dst, dtype=np.float32).view(np.uint8).reshape(-1)
    return torch.from_numpy(dst).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint8).reshape(-1)


@pytest.mark.parametrize("dt", E.DTYPES)
def test_pack_weights_all_against_the_layout_formula(dev, dt):
    """Every byte of every pack, padding included, and the guard gaps between the packs, after a 0xFF (NaN pattern) pre-fill."""
    from flair_amd import ops
    B.check_pack_table()
    descs, nfl, nby = B.pack_table(dt)
    params = B.pack_params(nfl)
    arena = torch.full((nby,), 0xFF, dtype=torch.uint8, device=dev)
    fields = lambda d: {k: v for k, v in d.items() if k not in ("name", "branch")}
    _, ran = _profiled(lambda: ops.pack_weights(dt, params.to(dev), [fields(d) for d in descs], arena))
    assert ran == {"pack_weights_all": 1}, ran
    got = arena.cpu().numpy()
    want = np.full(nby, 0xFF, dtype=np.uint8)
    for d in descs:
        b = _pack_bytes(B.pack_expected(d, params), dt)
        want[d["dst_off"]:d["dst_off"] + b.size] = b
    for d in descs:
        lo, hi = d["dst_off"], d["dst_off"] + d["rows_pad"] * d["Kpad"] * (4 if dt == "f32" else 2)
        bad = np.nonzero(got[lo:hi] != want[lo:hi])[0]
        es = 4 if dt == "f32" else 2
        assert bad.size == 0, (d["name"], d["branch"], f"{bad.size} bytes differ, first at element (row, col) =",
                               divmod(int(bad[0]) // es, d["Kpad"]), "last", divmod(int(bad[-1]) // es, d["Kpad"]))
    assert np.array_equal(got, want), "bytes outside the packs were written"
    # pack_weight, the single-layer packer every other operator test relies on, for the descriptors it can express (no tap subset):
    # the same bytes as pack_weights_all and as the formula, padding included, and nothing past rows_pad x Kpad elements
    es = 4 if dt == "f32" else 2
    pdev = params.to(dev)
    full = [d for d in descs if d["Rc"] == 0]
    assert len(full) >= 10 and {d["tf"] for d in full} == {0, 1}
    for d in full:
        nb = d["rows_pad"] * d["Kpad"] * es
        one = torch.full((nb + 256,), 0xFF, dtype=torch.uint8, device=dev)
        w = pdev[d["w_off"]:d["w_off"] + d["Cout"] * d["Cin"] * d["R"] * d["S"]]
        ops.pack_weight(dt, w, one, d["Cout"], d["Cin"], d["R"], d["S"], d["Cin_p"], d["rows_pad"], d["Kpad"], d["tf"])
        one = one.cpu().numpy()
        lo = d["dst_off"]
        for other, what in ((got[lo:lo + nb], "pack_weights_all"), (_pack_bytes(B.pack_expected(d, params), dt), "the layout formula")):
            bad = np.nonzero(one[:nb] != other)[0]
            assert bad.size == 0, (d["name"], "pack_weight against " + what, f"{bad.size} bytes differ, first at element (row, col) =",
                                   divmod(int(bad[0]) // es, d["Kpad"]))
        assert (one[nb:] == 0xFF).all(), (d["name"], "pack_weight wrote past its pack")


def test_pack_weights_refusals(dev):
    from flair_amd import ops
    p = torch.zeros(16384, device=dev)
    arena = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    ok = dict(w_off=0, dst_off=0, Cout=16, Cin=16, R=3, S=3, Cin_p=16, rows_pad=16, Kpad=160, tf=0)
    assert ops.pack_weights("f32", p, [ok] * 65, arena, rc=True) == -2
    assert ops.pack_weights("f32", p, [dict(ok, Kpad=128)], arena, rc=True) == -2     # a row shorter than its nine taps
    assert ops.pack_weights("f32", p, [ok], arena, rc=True) == 0
    # the 16-byte loads of the bf16 3x3 branches: a master that is not 16-byte aligned is refused, the element-wise branches take it
    bf = dict(ok, Kpad=192)
    tr = dict(w_off=0, dst_off=0, Cout=32, Cin=32, R=3, S=3, Cin_p=32, rows_pad=32, Kpad=320, tf=1)
    assert ops.pack_weights("bf16", p, [dict(bf, w_off=2)], arena, rc=True) == -2
    assert ops.pack_weights("bf16", p, [dict(tr, w_off=1)], arena, rc=True) == -2
    assert ops.pack_weights("bf16", p[1:], [bf], arena, rc=True) == -2
    assert ops.pack_weights("bf16", p, [dict(bf, w_off=4), dict(tr, w_off=2400, dst_off=8192)], arena, rc=True) == 0
    assert ops.pack_weights("f32", p, [dict(ok, w_off=2)], arena, rc=True) == 0
    assert ops.pack_weights("bf16", p, [dict(bf, Cin=15, w_off=2)], arena, rc=True) == 0
    # pack_weight holds its own real region too
    one = torch.zeros(16 * 160 * 4, dtype=torch.uint8, device=dev)
    assert ops.pack_weight("f32", p, one, 16, 16, 3, 3, 16, 16, 128, 0, rc=True) == -2
    assert ops.pack_weight("f32", p, one, 16, 16, 3, 3, 8, 16, 160, 0, rc=True) == -2
    assert ops.pack_weight("f32", p, one, 16, 16, 3, 3, 16, 8, 160, 1, rc=True) == -2
    assert ops.pack_weight("f32", p, one, 16, 16, 3, 3, 16, 16, 160, 0, rc=True) == 0


# ------------------------------------------------------------------------------------------------ f. max-pool family
@pytest.fixture(scope="module")
def pool_ref():
    """fp64 references of the pooling tests, once per channel count: x in {0, 1} (ties in every window)."""
    out = {}
    N, H, W = B.POOL_SHAPE
    for Cc in B.POOL_CHANNELS:
        g = torch.Generator().manual_seed(Cc)
        x = torch.relu(E.ternary((N, Cc, H, W), g, 0.5)).double().requires_grad_(True)
        p = F.max_pool2d(x, 3, 2, 1)
        dy = E.ternary(tuple(p.shape), g, 0.5)
        p.backward(dy.double())
        prev = E.ints((N, Cc, H, W), g, -8, 8)
        y, scale, shift, _, m = B.mask_inputs(g, (N, Cc, H, W), False)
        B.check_mask_variety("pool", y, scale, shift)
        ya = E.ints((N, Cc, H, W), g, -3, 3)
        sc, sh = E.ints((Cc,), g, -2, 2), E.ints((Cc,), g, -1, 1)
        act = torch.relu(ya.double() * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
        out[Cc] = dict(x=x.detach(), dy=dy, dx=x.grad, prev=prev, y=y, scale=scale, shift=shift, m=m, ya=ya, sc=sc, sh=sh, act=act,
                       pooled=F.max_pool2d(act, 3, 2, 1))
    return out


@pytest.mark.parametrize("dt", E.DTYPES)
@pytest.mark.parametrize("Cc", B.POOL_CHANNELS)
def test_maxpool_backward_accumulate_and_fused_reduction(dev, dt, Cc, pool_ref):
    from flair_amd import ops
    B.check_elementwise_shapes()
    N, H, W = B.POOL_SHAPE
    r = pool_ref[Cc]
    _, idx = ops.maxpool_forward(_nhwc(r["x"].float(), dt, dev))
    dy = _nhwc(r["dy"], dt, dev)
    din = _nhwc(r["prev"], dt, dev)
    _, ran = _profiled(lambda: ops.maxpool_backward_ex(dy, idx, H, W, dx=din, accumulate=True))
    assert ran == {"maxpool_bwd": 1}, ran
    _same(_nchw(din), r["dx"] + r["prev"].double(), "din += max pool backward")
    # fused reduction, on its own and on top of an accumulate: the sums are those of the STORED gradient
    for acc in (False, True):
        g = r["dx"] + (r["prev"].double() if acc else 0)
        din = _nhwc(r["prev"], dt, dev) if acc else torch.full((N, H, W, Cc), SENTINEL, dtype=TDT[dt], device=dev)
        part = torch.full((2, Cc, N * H), NAN, device=dev)
        y = _nhwc(r["y"], dt, dev)
        ops.maxpool_backward_ex(dy, idx, H, W, dx=din, accumulate=acc, bnr_y=y, bnr_msc=r["scale"].to(dev), bnr_msh=r["shift"].to(dev),
                                bnr_partial=part)
        _same(_nchw(din), g, "din with the fused reduction on")
        assert not bool(torch.isnan(part).any())
        gm = g * r["m"]
        # one partial row per input row (n, h)
        _same(part[0].double().t().reshape(N, H, Cc), gm.sum(3).permute(0, 2, 1), "sum g m per input row")
        _same(part[1].double().t().reshape(N, H, Cc), (gm * r["y"].double()).sum(3).permute(0, 2, 1), "sum g m y per input row")


@pytest.mark.parametrize("dt", E.DTYPES)
@pytest.mark.parametrize("Cc", B.POOL_CHANNELS)
def test_bn_act_maxpool_is_bn_act_then_maxpool(dev, dt, Cc, pool_ref):
    from flair_amd import ops
    N, H, W = B.POOL_SHAPE
    r = pool_ref[Cc]
    y = _nhwc(r["ya"], dt, dev)
    sc, sh = r["sc"].to(dev), r["sh"].to(dev)
    (act, pooled, idx), ran = _profiled(lambda: ops.bn_act_maxpool(y, sc, sh))
    assert ran == {"bn_act_maxpool": 1}, ran
    act2 = ops.bn_act(y, sc, sh)
    pooled2, idx2 = ops.maxpool_forward(act2)
    assert torch.equal(act, act2) and torch.equal(pooled, pooled2) and torch.equal(idx, idx2)
    _same(_nchw(act), r["act"], "relu(y scale + shift)")
    _same(_nchw(pooled), r["pooled"], "its 3x3 / stride-2 max pool")
    # the tap indices against plain indexing: first maximum of the window in (kh, kw) scan order
    a = F.pad(r["act"], (1, 1, 1, 1), value=float("-inf")).unfold(2, 3, 2).unfold(3, 3, 2).reshape(N, Cc, H // 2, W // 2, 9)
    first = (a == a.amax(4, keepdim=True)).double().argmax(4)
    _same(idx.permute(0, 3, 1, 2), first, "tap index of the first maximum")


def test_pool_refusals(dev):
    from flair_amd import ops
    odd = torch.zeros(1, 5, 8, 16, device=dev)
    v = torch.ones(16, device=dev)
    idx = torch.zeros(1, 3, 4, 16, dtype=torch.uint8, device=dev)
    assert ops.bn_act_maxpool(odd, v, v, rc=True) == -2
    assert ops.maxpool_backward_ex(torch.zeros(1, 3, 4, 16, device=dev), idx, 5, 8, rc=True) == -2
    assert ops.maxpool_backward_ex(torch.zeros(1, 3, 4, 16, device=dev), idx, 6, 7, rc=True) == -2
    dy = torch.zeros(1, 3, 4, 24, device=dev, dtype=torch.bfloat16)                # three chunk columns: 256 % 3 != 0
    part = torch.full((2, 24, 6), NAN, device=dev)
    v24 = torch.ones(24, device=dev)
    rc = ops.maxpool_backward_ex(dy, torch.zeros(1, 3, 4, 24, dtype=torch.uint8, device=dev), 6, 8,
                                 bnr_y=torch.zeros(1, 6, 8, 24, device=dev, dtype=torch.bfloat16), bnr_msc=v24, bnr_msh=v24, bnr_partial=part, rc=True)
    assert rc == -2 and bool(torch.isnan(part).all())


# ------------------------------------------------------------------------------------------------ g. upcat_bwd, ew_add, colsum
@pytest.mark.parametrize("dt", E.DTYPES)
@pytest.mark.parametrize("shape", B.UPCAT_CASES, ids=lambda s: "x".join(map(str, s)))
def test_upcat_bwd_all_accumulate_combinations(dev, dt, shape):
    from flair_amd import ops
    N, H, W, C0, C1 = shape
    g = torch.Generator().manual_seed(H + C1)
    dcat = E.ints((N, C0 + C1, H, W), g, -8, 8)
    p0, p1 = E.ints((N, C0, H // 2, W // 2), g, -8, 8), E.ints((N, C1, H, W), g, -8, 8)
    pooled = F.avg_pool2d(dcat[:, :C0].double(), 2) * 4
    dk = _nhwc(dcat, dt, dev)
    for a0, a1 in ((False, False), (False, True), (True, False), (True, True)):
        dx0 = _nhwc(p0, dt, dev) if a0 else torch.full((N, H // 2, W // 2, C0), SENTINEL, dtype=TDT[dt], device=dev)
        dsk = None if not C1 else _nhwc(p1, dt, dev) if a1 else torch.full((N, H, W, C1), SENTINEL, dtype=TDT[dt], device=dev)
        _, ran = _profiled(lambda: ops.upcat_bwd(dk, C0, dx0=dx0, dx0_accumulate=a0, dskip=dsk, dskip_accumulate=a1))
        assert ran == {"upcat_bwd": 1}, ran
        _same(_nchw(dx0), pooled + (p0.double() if a0 else 0), f"dx0 (accumulate {a0}, {a1})")
        if C1:
            _same(_nchw(dsk), dcat[:, C0:].double() + (p1.double() if a1 else 0), f"dskip (accumulate {a0}, {a1})")


@pytest.mark.parametrize("dt", E.DTYPES)
def test_ew_add_and_colsum(dev, dt):
    from flair_amd import ops
    ch = 4 if dt == "f32" else 8
    g = torch.Generator().manual_seed(7)
    n = 256 * ch * 3 + 5 * ch                      # no multiple of one workgroup's 256 chunks
    a, b = E.ints((n + ch,), g, -100, 100), E.ints((n + ch,), g, -100, 100)
    d = a.to(device=dev, dtype=TDT[dt])
    ops.ew_add_(d, b.to(device=dev, dtype=TDT[dt]), n=n)
    want = a.double().clone()
    want[:n] += b[:n].double()                     # the chunk past n keeps its value
    _same(d, want, "dst[:n] += src[:n]")
    assert ops.ew_add_(d, d.clone(), n=n - 1, rc=True) == -2
    rows, ld, Cc = B.COLSUM_CASE
    x = E.ternary((rows, ld), g, 0.5)
    x[-1, :] = 1                                   # the ragged last row counts
    _same(ops.colsum(x.to(device=dev, dtype=TDT[dt]), Cc), x[:, :Cc].double().sum(0), "column sums, first C of ld columns")


# ------------------------------------------------------------------------------------------------ h. stem weight gradient, fused apply
@pytest.mark.parametrize("shape", B.STEM_CASES, ids=lambda s: "x".join(map(str, s)))
def test_stem_wgrad_fused_apply_exact(dev, shape):
    """bf16 only (the stem kernels exist in bf16).  Integer coefficients: the staged k1 dz + k2 y + k3 is an exact bf16 integer and
    dw equals the fp64 weight gradient of that tensor."""
    from flair_amd import ops
    r = B.stem_reference(shape)
    name = B.check_stem_dispatch(shape)[1]
    x, dout, y = (_nhwc(r[k], "bf16", dev) for k in ("x", "dout", "y"))
    dw = torch.full((64, 5, 7, 7), NAN, device=dev)
    _, ran = _profiled(lambda: ops.conv2d_wgrad_ex(x, dout, 64, R=7, stride=2, pad=3, cin_real=5, dw=dw, fuse_y=y, fuse_coef=r["coef"].to(dev),
                                                   fuse_msc=r["scale"].to(dev), fuse_msh=r["shift"].to(dev)))
    assert ran == {name: 1}, ran
    _same(dw, r["dw"], "dw of the fused apply")
    # and the same tensor materialised: the plain stem kernel on the staged gradient
    dw2, _ = ops.conv2d_wgrad_ex(x, _nhwc(r["staged"].float(), "bf16", dev), 64, R=7, stride=2, pad=3, cin_real=5)
    assert torch.equal(dw, dw2)


@pytest.mark.parametrize("shape", B.STEM_CASES, ids=lambda s: "x".join(map(str, s)))
def test_stem_wgrad_fused_apply_matches_the_separate_pass(dev, shape):
    """Real coefficients: bn_backward (dy == nullptr) leaves k1 | k2 | k3, the fused kernel applies them while it stages dy; the
    unfused route writes dy with bn_bwd_apply and runs the plain kernel.  Same rounding, same order: the same bits."""
    from flair_amd import ops
    r = B.stem_reference(shape)
    x, dout, y = (_nhwc(r[k], "bf16", dev) for k in ("x", "dout", "y"))
    g = torch.Generator().manual_seed(11)
    mean, invstd, gamma = (torch.rand(64, generator=g) - 0.5).to(dev), (torch.rand(64, generator=g) + 0.5).to(dev), (torch.rand(64, generator=g) + 0.5).to(dev)
    msc, msh = r["scale"].to(dev), r["shift"].to(dev)
    rows2d = lambda t: t.reshape(-1, 64)
    only = ops.bn_backward_ex(rows2d(dout), rows2d(y), mean, invstd, gamma=gamma, mscale=msc, mshift=msh, want_dy=False)
    both = ops.bn_backward_ex(rows2d(dout), rows2d(y), mean, invstd, gamma=gamma, mscale=msc, mshift=msh)
    assert torch.equal(only["coef"], both["coef"]) and torch.equal(only["dgamma"], both["dgamma"])
    fused, _ = ops.conv2d_wgrad_ex(x, dout, 64, R=7, stride=2, pad=3, cin_real=5, fuse_y=y, fuse_coef=only["coef"], fuse_msc=msc, fuse_msh=msh)
    plain, _ = ops.conv2d_wgrad_ex(x, both["dy"].view_as(dout), 64, R=7, stride=2, pad=3, cin_real=5)
    assert torch.equal(fused, plain), float((fused - plain).abs().max())
    assert float(plain.abs().max()) > 0


def test_stem_fused_apply_is_refused_elsewhere(dev):
    from flair_amd import ops
    from flair_amd._lib import FlairHipError
    x = torch.zeros(1, 16, 64, 16, device=dev, dtype=torch.bfloat16)
    with pytest.raises(FlairHipError, match=r"code -6"):
        ops.conv2d_wgrad_ex(x, x, 16, fuse_y=x, fuse_coef=torch.zeros(3, 16, device=dev), fuse_msc=torch.ones(16, device=dev),
                            fuse_msh=torch.ones(16, device=dev))
