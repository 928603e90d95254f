"""Operator-level wrappers over the C ABI (used by the parity tests and by host code).

Activations are NHWC tensors in the compute dtype (torch.float32 / torch.bfloat16); weights are
PyTorch OIHW fp32.  Every call goes through libflair_hip.so; nothing here computes on the host.
"""
from __future__ import annotations

import torch

from . import _lib as L


def _ws(nbytes, device):
    return torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)


def _dt(t):
    return L.dtype_code(t.dtype)


def nchw_to_nhwc(x: torch.Tensor, dtype, cpad=None) -> torch.Tensor:
    N, C, H, W = x.shape
    dt = L.dtype_code(dtype)
    cpad = cpad or ((C + 7) // 8 * 8)
    y = torch.empty(N, H, W, cpad, dtype=L.torch_dtype(dt), device=x.device)
    L.check(L.lib().flair_nchw_to_nhwc(dt, L.ptr(x.float().contiguous()), L.ptr(y), N, C, H, W, cpad, L.stream()), "nchw_to_nhwc")
    return y


def nhwc_to_nchw(x: torch.Tensor, C=None) -> torch.Tensor:
    N, H, W, Cp = x.shape
    C = C or Cp
    y = torch.empty(N, C, H, W, dtype=torch.float32, device=x.device)
    L.check(L.lib().flair_nhwc_to_nchw(_dt(x), L.ptr(x), L.ptr(y), N, C, H, W, Cp, L.stream()), "nhwc_to_nchw")
    return y


def conv2d_forward(x0, w, bias=None, stride=1, pad=1, x1=None, up0=False, want_nchw=False, want_stats=False):
    """y = conv2d(cat([up2(x0) if up0 else x0, x1], C), w) on NHWC inputs; returns (y_nhwc, y_nchw, stats)."""
    N, H, W, C0 = x0.shape
    C1 = x1.shape[3] if x1 is not None else 0
    Cout, Cin, R, _ = w.shape
    assert Cin == C0 + C1
    dt = _dt(x0)
    Hin, Win = (2 * H, 2 * W) if up0 else (H, W)
    Ho, Wo = (Hin + 2 * pad - R) // stride + 1, (Win + 2 * pad - R) // stride + 1
    l = L.lib()
    ws = _ws(l.flair_conv2d_workspace_bytes(dt, N, H, W, C0, C1, int(up0), Cout, R, stride, pad), x0.device)
    y = torch.empty(N, Ho, Wo, Cout, dtype=x0.dtype, device=x0.device) if Cout % 8 == 0 else None
    yn = torch.empty(N, Cout, Ho, Wo, dtype=torch.float32, device=x0.device) if (want_nchw or y is None) else None
    st = torch.empty(2, Cout, dtype=torch.float32, device=x0.device) if want_stats else None
    L.check(l.flair_conv2d_forward(dt, L.ptr(x0), L.ptr(x1), N, H, W, C0, C1, int(up0), L.ptr(w), L.ptr(bias), Cout, R,
                                   stride, pad, L.ptr(y), L.ptr(yn), L.ptr(st), L.ptr(ws), ws.numel(), L.stream()),
            "conv2d_forward")
    return y, yn, st


def conv2d_backward(x, w, dy, stride=1, pad=1, need_dx=True, need_dw=True):
    N, H, W, Cin = x.shape
    Cout, _, R, _ = w.shape
    dt = _dt(x)
    l = L.lib()
    ws = _ws(l.flair_conv2d_workspace_bytes(dt, N, H, W, Cin, 0, 0, Cout, R, stride, pad), x.device)
    dx = torch.empty_like(x) if need_dx else None
    dw = torch.empty_like(w) if need_dw else None
    L.check(l.flair_conv2d_backward(dt, L.ptr(x), N, H, W, Cin, L.ptr(w), Cout, R, stride, pad, L.ptr(dy), L.ptr(dx),
                                    L.ptr(dw), L.ptr(ws), ws.numel(), L.stream()), "conv2d_backward")
    return dx, dw


def _conv_ex_args(x0, w, mode=0, bias=None, stride=1, pad=1, x1=None, up0=False, want_nhwc=True, want_nchw=False, want_stats=False,
                  in_scale=None, in_shift=None, oscale=None, oshift=None, ores=None, orelu=False, out=None, accumulate=False,
                  acc_src=None, pool_c0=0, out_skip=None, skip_accumulate=False, want_preds=False, want_maxprob=False, ogelu=False,
                  bnr_y=None, bnr_out=None, bnr_scale=None, bnr_shift=None, bnr_partial=None, bnr_mask=False):
    """(flair_conv_ex_t, outputs) of conv2d_ex / conv2d_ex_grid_rows.  The library picks its kernel from which pointers are set, so
    the sizing query gets the same struct, outputs included, as the launch."""
    N, H, W, C0 = x0.shape
    C1 = x1.shape[3] if x1 is not None else 0
    R = w.shape[2]
    Cout = w.shape[1] if mode else w.shape[0]
    assert (w.shape[0] if mode else w.shape[1]) == C0 + C1
    dt = _dt(x0)
    Hin, Win = (2 * H, 2 * W) if up0 else (H, W)
    p_eff = R - 1 - pad if mode == 1 else pad
    Ho, Wo = (Hin + 2 * p_eff - R) // stride + 1, (Win + 2 * p_eff - R) // stride + 1
    dev = x0.device
    if mode == 2:
        assert out is not None, "mode 2 writes into the caller's dx"
        Ho, Wo = H, W
    if out is None and want_nhwc:
        assert not accumulate or acc_src is not None, "accumulate needs the tensor to add to"
        out = (torch.empty(N, Ho // 2, Wo // 2, pool_c0, dtype=x0.dtype, device=dev) if pool_c0 else
               torch.empty(N, Ho, Wo, Cout, dtype=x0.dtype, device=dev))
    if pool_c0 and pool_c0 < Cout and out_skip is None:
        assert not skip_accumulate
        out_skip = torch.empty(N, Ho, Wo, Cout - pool_c0, dtype=x0.dtype, device=dev)
    yn = torch.empty(N, Cout, Ho, Wo, dtype=torch.float32, device=dev) if want_nchw else None
    st = torch.empty(2, Cout, dtype=torch.float32, device=dev) if want_stats else None
    pr = torch.empty(N, Ho, Wo, dtype=torch.uint8, device=dev) if want_preds else None
    mp = torch.empty(N, Ho, Wo, dtype=torch.float32, device=dev) if want_maxprob else None
    a = L.ConvEx(dtype=dt, mode=mode, x0=L.ptr(x0), x1=L.ptr(x1), N=N, H=H, W=W, C0=C0, C1=C1, up0=int(up0), w_oihw=L.ptr(w),
                 bias=L.ptr(bias), Cout=Cout, R=R, stride=stride, pad=pad, y_nhwc=L.ptr(out),
                 out_ld=out.shape[3] if out is not None else 0, y_nchw=L.ptr(yn), stats=L.ptr(st), in_scale=L.ptr(in_scale),
                 in_shift=L.ptr(in_shift), oscale=L.ptr(oscale), oshift=L.ptr(oshift), ores=L.ptr(ores), orelu=int(orelu),
                 accumulate=int(accumulate), acc_src=L.ptr(acc_src), pool_c0=pool_c0, out_skip=L.ptr(out_skip),
                 out_skip_ld=out_skip.shape[3] if out_skip is not None else 0, skip_accumulate=int(skip_accumulate),
                 preds_u8=L.ptr(pr), maxprob_f32=L.ptr(mp), ogelu=int(ogelu),
                 bnr_y=L.ptr(bnr_y), bnr_out=L.ptr(bnr_out), bnr_scale=L.ptr(bnr_scale), bnr_shift=L.ptr(bnr_shift),
                 bnr_partial=L.ptr(bnr_partial), bnr_rows=bnr_partial.shape[2] if bnr_partial is not None else 0, bnr_mask=int(bnr_mask))
    return a, {"y": out, "out_skip": out_skip, "y_nchw": yn, "stats": st, "preds": pr, "maxprob": mp}


def conv2d_ex(x0, w, **kw):
    """flair_conv2d_ex: the fused forms of the convolution launcher (keywords: those of _conv_ex_args).
    mode 0: forward, w = [Cout][C0 + C1][R][R]; mode 1: stride-1 data gradient, x0 = dy, w = the forward layer's [C0][Cout][R][R].  `out` (NHWC, optional) is the tensor accumulated into / written;
    with pool_c0 it is [N][H/2][W/2][pool_c0] and out_skip [N][H][W][Cout - pool_c0].  ogelu: erf-GELU of the
    accumulator (+ bias) before ores / orelu (gather-form GEMM only).
    mode 2: the stride-2 data gradient by parity class, x0 = dy, w as in mode 1, `out` = dx [N][2H][2W][Cout] (required).
    bnr_partial (fp32 [2][out_ld][rows], rows >= conv2d_ex_grid_rows(...)): the fused BatchNorm-backward reduction of the epilogue
    against bnr_y (and bnr_scale / bnr_shift, or bnr_out); bnr_mask stores the masked gradient.
    Returns a dict: y, out_skip, y_nchw, stats, preds, maxprob (absent outputs None)."""
    import ctypes as C
    a, outs = _conv_ex_args(x0, w, **kw)
    l = L.lib()
    ws = _ws(l.flair_conv2d_ex_workspace_bytes(C.addressof(a)), x0.device)
    L.check(l.flair_conv2d_ex(C.addressof(a), L.ptr(ws), ws.numel(), L.stream()), "conv2d_ex")
    return outs


def conv2d_ex_grid_rows(x0, w, **kw):
    """flair_conv2d_ex_grid_rows for the arguments of conv2d_ex (nothing is launched): the row blocks of stats / bnr_partial.
    Pass bnr_y to ask for the launch WITH the fused reduction."""
    import ctypes as C
    a, _ = _conv_ex_args(x0, w, **kw)
    rows = L.lib().flair_conv2d_ex_grid_rows(C.addressof(a))
    L.check(min(rows, 0), "conv2d_ex_grid_rows")
    return rows


def conv2d_wgrad_ex(x0, dy, Cout, R=3, stride=1, pad=1, x1=None, up0=False, in_scale=None, in_shift=None, dw=None, accumulate=False,
                    want_dbias=False, cus=0, cin_real=0, fuse_y=None, fuse_coef=None, fuse_msc=None, fuse_msh=None):
    """flair_conv2d_wgrad_ex: dw (and the fused dbias) of conv(cat([up2(x0)?, x1])) against dy [N][Ho][Wo][dy_ld >= Cout].
    fuse_y / fuse_coef (k1 | k2 | k3) / fuse_msc / fuse_msh: the stem kernel's fused BatchNorm-backward apply on dy."""
    import ctypes as C
    N, H, W, C0 = x0.shape
    C1 = x1.shape[3] if x1 is not None else 0
    dt = _dt(x0)
    dev = x0.device
    if dw is None:
        assert not accumulate
        dw = torch.empty(Cout, cin_real or (C0 + C1), R, R, dtype=torch.float32, device=dev)
    db = torch.empty(Cout, dtype=torch.float32, device=dev) if want_dbias else None
    a = L.WgradEx(dtype=dt, x0=L.ptr(x0), x1=L.ptr(x1), N=N, H=H, W=W, C0=C0, C1=C1, up0=int(up0), dy=L.ptr(dy), dy_ld=dy.shape[3],
                  Cout=Cout, R=R, stride=stride, pad=pad, dw=L.ptr(dw), Cin_real=cin_real, accumulate=int(accumulate),
                  in_scale=L.ptr(in_scale), in_shift=L.ptr(in_shift), dbias=L.ptr(db), cus=cus,
                  fuse_y=L.ptr(fuse_y), fuse_coef=L.ptr(fuse_coef), fuse_msc=L.ptr(fuse_msc), fuse_msh=L.ptr(fuse_msh))
    l = L.lib()
    ws = _ws(l.flair_conv2d_wgrad_ex_workspace_bytes(C.addressof(a)), dev)
    L.check(l.flair_conv2d_wgrad_ex(C.addressof(a), L.ptr(ws), ws.numel(), L.stream()), "conv2d_wgrad_ex")
    return dw, db


def bn_relu_forward(y, gamma, beta, running_mean, running_var, training=True, residual=None, relu=True):
    C = y.shape[-1]
    rows = y.numel() // C
    out = torch.empty_like(y)
    mean = torch.empty(C, dtype=torch.float32, device=y.device)
    invstd = torch.empty(C, dtype=torch.float32, device=y.device)
    ws = _ws(L.lib().flair_bn_workspace_bytes(rows, C), y.device)
    L.check(L.lib().flair_bn_relu_forward(_dt(y), L.ptr(y), rows, C, L.ptr(gamma), L.ptr(beta), L.ptr(running_mean),
                                          L.ptr(running_var), int(training), L.ptr(residual), int(relu), L.ptr(out),
                                          L.ptr(mean), L.ptr(invstd), L.ptr(ws), ws.numel(), L.stream()), "bn_relu_forward")
    return out, mean, invstd


def bn_relu_backward(dout, out, y, gamma, mean, invstd, relu=True, want_dres=False):
    C = y.shape[-1]
    rows = y.numel() // C
    dy = torch.empty_like(y)
    dres = torch.empty_like(y) if want_dres else None
    dgamma = torch.empty(C, dtype=torch.float32, device=y.device)
    dbeta = torch.empty(C, dtype=torch.float32, device=y.device)
    ws = _ws(L.lib().flair_bn_workspace_bytes(rows, C), y.device)
    L.check(L.lib().flair_bn_relu_backward(_dt(y), L.ptr(dout), L.ptr(out), L.ptr(y), rows, C, L.ptr(gamma), L.ptr(mean),
                                           L.ptr(invstd), int(relu), L.ptr(dy), L.ptr(dres), L.ptr(dgamma), L.ptr(dbeta),
                                           L.ptr(ws), ws.numel(), L.stream()), "bn_relu_backward")
    return dy, dres, dgamma, dbeta


def bn_backward_ex(dout, y, mean, invstd, gamma=None, out=None, mscale=None, mshift=None, partial=None, pre_nblk=0, premasked=False,
                   dgamma=None, dbeta=None, accumulate_param=False, want_dy=True, dy=None, dres=None, want_dres=False,
                   dres_accumulate=False, coef=None, rc=False):
    """flair_bn_backward_ex: bn_backward as the network calls it.  partial [2][C][pre_nblk] fp32 with pre_nblk > 0: the producer's
    block sums; dy, dgamma / dbeta, coef are allocated unless given (accumulate_param adds into dgamma / dbeta); dres given or want_dres.
    Returns a dict: dy, dres, dgamma, dbeta, coef [3][C]."""
    import ctypes as C
    Cc = y.shape[-1]
    rows = y.numel() // Cc
    dev = y.device
    if dy is None and want_dy:
        dy = torch.empty_like(y)
    if dres is None and want_dres:
        assert not dres_accumulate
        dres = torch.empty_like(y)
    if dgamma is None:
        assert not accumulate_param
        dgamma = torch.empty(Cc, dtype=torch.float32, device=dev)
        dbeta = torch.empty(Cc, dtype=torch.float32, device=dev)
    if coef is None:
        coef = torch.empty(3, Cc, dtype=torch.float32, device=dev)
    a = L.BnBwdEx(dtype=_dt(y), dout=L.ptr(dout), out=L.ptr(out), y=L.ptr(y), mean=L.ptr(mean), invstd=L.ptr(invstd), gamma=L.ptr(gamma),
                  rows=rows, C=Cc, partial=L.ptr(partial), pre_nblk=pre_nblk, premasked=int(premasked), mscale=L.ptr(mscale),
                  mshift=L.ptr(mshift), dgamma=L.ptr(dgamma), dbeta=L.ptr(dbeta), accumulate_param=int(accumulate_param), dy=L.ptr(dy),
                  dres=L.ptr(dres), dres_accumulate=int(dres_accumulate), coef=L.ptr(coef))
    ws = _ws(L.lib().flair_bn_workspace_bytes(rows, Cc), dev)
    r = L.lib().flair_bn_backward_ex(C.addressof(a), L.ptr(ws), ws.numel(), L.stream())
    return _ret(r, "bn_backward_ex", {"dy": dy, "dres": dres, "dgamma": dgamma, "dbeta": dbeta, "coef": coef}, rc)


def bwd16_ex(g, x, in_scale, in_shift, w, bnr_scale, bnr_shift, gy=None, gcoef=None, gmsc=None, gmsh=None, want_dbias=False, rc=False):
    """flair_bwd16_ex: the fused backward of a 16 -> <= 16 channel 3x3 layer (bf16 NHWC tensors of 16 channels; w the forward layer's
    [Cout][16][3][3]).  gy / gcoef / gmsc / gmsh: the unit flavour (g is then the gradient w.r.t. the unit's ReLU output).
    Returns a dict: dx, dw, dbias (None unless want_dbias), partial [2][16][rows] (the fused BatchNorm-backward sums), rows."""
    import ctypes as C
    N, H, W, _ = g.shape
    dev = g.device
    Cout = w.shape[0]
    a = L.Bwd16Ex(g=L.ptr(g), gy=L.ptr(gy), gcoef=L.ptr(gcoef), gmsc=L.ptr(gmsc), gmsh=L.ptr(gmsh), x=L.ptr(x), in_scale=L.ptr(in_scale),
                  in_shift=L.ptr(in_shift), w_oihw=L.ptr(w), Cout=Cout, N=N, H=H, W=W, bnr_scale=L.ptr(bnr_scale), bnr_shift=L.ptr(bnr_shift))
    l = L.lib()
    rows = l.flair_bwd16_ex_grid_rows(C.addressof(a))
    if rows < 0:
        return _ret(rows, "bwd16_ex_grid_rows", None, rc)
    dx = torch.full_like(g, float("nan"))
    dw = torch.full((Cout, 16, 3, 3), float("nan"), dtype=torch.float32, device=dev)
    db = torch.full((Cout,), float("nan"), dtype=torch.float32, device=dev) if want_dbias else None
    part = torch.full((2, 16, rows), float("nan"), dtype=torch.float32, device=dev)
    a.dx, a.dw, a.dbias, a.bnr_partial, a.bnr_rows = L.ptr(dx), L.ptr(dw), L.ptr(db), L.ptr(part), rows
    ws = _ws(l.flair_bwd16_ex_workspace_bytes(C.addressof(a)), dev)
    r = l.flair_bwd16_ex(C.addressof(a), L.ptr(ws), ws.numel(), L.stream())
    return _ret(r, "bwd16_ex", {"dx": dx, "dw": dw, "dbias": db, "partial": part, "rows": rows}, rc)


def maxpool_backward_ex(dy, idx, H, W, dx=None, accumulate=False, bnr_y=None, bnr_msc=None, bnr_msh=None, bnr_partial=None, rc=False):
    """flair_maxpool_backward_ex: dx (+= with accumulate); bnr_partial fp32 [2][C][N * H] receives the fused reduction."""
    N, _, _, Cc = dy.shape
    if dx is None:
        assert not accumulate
        dx = torch.empty(N, H, W, Cc, dtype=dy.dtype, device=dy.device)
    r = L.lib().flair_maxpool_backward_ex(_dt(dy), L.ptr(dy), L.ptr(idx), L.ptr(dx), int(accumulate), N, H, W, Cc, L.ptr(bnr_y),
                                          L.ptr(bnr_msc), L.ptr(bnr_msh), L.ptr(bnr_partial), L.stream())
    return _ret(r, "maxpool_backward_ex", dx, rc)


def bn_act_maxpool(y, scale, shift, rc=False):
    """flair_bn_act_maxpool: (act, pooled, idx) of relu(y * scale + shift) and its 3x3 / stride-2 max pool."""
    N, H, W, Cc = y.shape
    act = torch.empty_like(y)
    out = torch.empty(N, H // 2, W // 2, Cc, dtype=y.dtype, device=y.device)
    idx = torch.empty(N, H // 2, W // 2, Cc, dtype=torch.uint8, device=y.device)
    r = L.lib().flair_bn_act_maxpool(_dt(y), L.ptr(y), L.ptr(scale), L.ptr(shift), L.ptr(act), L.ptr(out), L.ptr(idx), N, H, W, Cc,
                                     L.stream())
    return _ret(r, "bn_act_maxpool", (act, out, idx), rc)


def bn_act(y, scale, shift, relu=True, rc=False):
    """flair_bn_act: [relu](y * scale + shift), the standalone pass bn_act_maxpool folds into the pool."""
    Cc = y.shape[-1]
    out = torch.empty_like(y)
    r = L.lib().flair_bn_act(_dt(y), L.ptr(y), L.ptr(scale), L.ptr(shift), L.ptr(out), y.numel() // Cc, Cc, int(relu), L.stream())
    return _ret(r, "bn_act", out, rc)


def upcat_bwd(dcat, C0, dx0=None, dx0_accumulate=False, dskip=None, dskip_accumulate=False, rc=False):
    """flair_upcat_bwd: dcat [N][H][W][C0 + C1] -> (dx0 [N][H/2][W/2][C0], dskip [N][H][W][C1] or None)."""
    N, H, W, Ct = dcat.shape
    C1 = Ct - C0
    if dx0 is None:
        assert not dx0_accumulate
        dx0 = torch.empty(N, H // 2, W // 2, C0, dtype=dcat.dtype, device=dcat.device)
    if dskip is None and C1:
        assert not dskip_accumulate
        dskip = torch.empty(N, H, W, C1, dtype=dcat.dtype, device=dcat.device)
    r = L.lib().flair_upcat_bwd(_dt(dcat), L.ptr(dcat), L.ptr(dx0), int(dx0_accumulate), L.ptr(dskip), int(dskip_accumulate), N, H, W,
                                C0, C1, L.stream())
    return _ret(r, "upcat_bwd", (dx0, dskip), rc)


def ew_add_(dst, src, n=None, rc=False):
    """flair_ew_add: dst[:n] += src[:n] in place (flat element count, default all)."""
    n = dst.numel() if n is None else n
    return _ret(L.lib().flair_ew_add(_dt(dst), L.ptr(dst), L.ptr(src), n, L.stream()), "ew_add", dst, rc)


def colsum(x, C, rc=False):
    """flair_colsum: fp32 [C] column sums of x [rows][ld], C <= ld."""
    rows, ld = x.shape
    out = torch.empty(C, dtype=torch.float32, device=x.device)
    ws = _ws(L.lib().flair_bn_workspace_bytes(rows, ld), x.device)
    r = L.lib().flair_colsum(_dt(x), L.ptr(x), rows, ld, C, L.ptr(out), L.ptr(ws), ws.numel(), L.stream())
    return _ret(r, "colsum", out, rc)


def pack_weights(dtype, params, descs, arena, rc=False):
    """flair_pack_weights: descs = list of dicts with the fields of flair_pack_desc_t (missing ones 0); params flat fp32, arena a
    uint8 tensor the dst_off byte offsets point into."""
    import ctypes as C
    arr = (L.PackDesc * len(descs))(*[L.PackDesc(**d) for d in descs])
    r = L.lib().flair_pack_weights(L.dtype_code(dtype), L.ptr(params), C.addressof(arr), len(descs), L.ptr(arena), L.stream())
    return _ret(r, "pack_weights", arena, rc)


def pack_weight(dtype, w, dst, Cout, Cin, R, S, Cin_p, rows_pad, Kpad, tf, rc=False):
    """flair_pack_weight: the single-layer packer of the operator entry points, w (fp32 OIHW) -> dst [rows_pad][Kpad] of `dtype`."""
    r = L.lib().flair_pack_weight(L.dtype_code(dtype), L.ptr(w), L.ptr(dst), Cout, Cin, R, S, Cin_p, rows_pad, Kpad, int(tf), L.stream())
    return _ret(r, "pack_weight", dst, rc)


def maxpool_forward(x):
    N, H, W, C = x.shape
    y = torch.empty(N, H // 2, W // 2, C, dtype=x.dtype, device=x.device)
    idx = torch.empty(N, H // 2, W // 2, C, dtype=torch.uint8, device=x.device)
    L.check(L.lib().flair_maxpool_forward(_dt(x), L.ptr(x), L.ptr(y), L.ptr(idx), N, H, W, C, L.stream()), "maxpool_forward")
    return y, idx


def maxpool_backward(dy, idx, H, W):
    N, _, _, C = dy.shape
    dx = torch.empty(N, H, W, C, dtype=dy.dtype, device=dy.device)
    L.check(L.lib().flair_maxpool_backward(_dt(dy), L.ptr(dy), L.ptr(idx), L.ptr(dx), N, H, W, C, L.stream()), "maxpool_backward")
    return dx


_LABEL_KIND = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}


def ce_head(logits, labels, weight=None, want_dlogits=True, want_preds="u8", confmat=None, want_targets=False,
            dlogits_nhwc=None, dlogits_ld=0):
    """Fused CE + argmax(softmax) + confusion matrix.  labels: (B,H,W) uint8/int32/int64 or fp32 one-hot (B,C,H,W)."""
    B, Cc, H, W = logits.shape
    kind = 3 if labels.dtype == torch.float32 else _LABEL_KIND[labels.dtype]
    dev = logits.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    dl = torch.empty_like(logits) if want_dlogits else None
    pu8 = torch.empty(B, H, W, dtype=torch.uint8, device=dev) if want_preds == "u8" else None
    pi64 = torch.empty(B, H, W, dtype=torch.int64, device=dev) if want_preds == "i64" else None
    tg = torch.empty(B, H, W, dtype=torch.int32, device=dev) if want_targets else None
    l = L.lib()
    ws = _ws(l.flair_ce_workspace_bytes(B, H, W), dev)
    L.check(l.flair_ce_head(L.ptr(logits), L.ptr(labels), kind, L.ptr(weight), B, Cc, H, W, L.ptr(loss), L.ptr(dl),
                            L.ptr(dlogits_nhwc), _dt(dlogits_nhwc) if dlogits_nhwc is not None else 0, dlogits_ld,
                            L.ptr(pu8), L.ptr(pi64), L.ptr(tg), L.ptr(confmat), L.ptr(ws), L.stream()), "ce_head")
    return loss, dl, (pu8 if pu8 is not None else pi64), tg


def seg_loss_spec(spec):
    """The flair_seg_loss_t of a ``flair_amd.losses.SegLoss`` (or of six floats in its field order: the operator tests)."""
    vals = spec.astuple() if hasattr(spec, "astuple") else tuple(spec)
    return L.SegLossSpec(*[float(v) for v in vals])


def seg_loss(logits, labels, spec, weight=None, want_dlogits=True, want_preds="u8", confmat=None, want_targets=False):
    """The head with a configurable objective (flair_seg_loss; ``spec``: a flair_amd.losses.SegLoss): loss = ce * CE + dice * Dice,
    its gradient, argmax(softmax) and the confusion matrix.  logits fp32 (B,C,H,W); labels as for ce_head.  Returns
    (terms, dlogits, preds, targets): terms a 3-float device tensor [loss, CE, Dice]."""
    import ctypes as C
    B, Cc, H, W = logits.shape
    kind = 3 if labels.dtype == torch.float32 else _LABEL_KIND[labels.dtype]
    dev = logits.device
    terms = torch.empty(3, dtype=torch.float32, device=dev)
    dl = torch.empty_like(logits) if want_dlogits else None
    pu8 = torch.empty(B, H, W, dtype=torch.uint8, device=dev) if want_preds == "u8" else None
    pi64 = torch.empty(B, H, W, dtype=torch.int64, device=dev) if want_preds == "i64" else None
    tg = torch.empty(B, H, W, dtype=torch.int32, device=dev) if want_targets else None
    l = L.lib()
    ws = _ws(l.flair_seg_loss_workspace_bytes(B, Cc, H, W), dev)
    sp = seg_loss_spec(spec)
    L.check(l.flair_seg_loss(L.ptr(logits), L.ptr(labels), kind, L.ptr(weight), B, Cc, H, W, C.byref(sp), L.ptr(terms), L.ptr(dl),
                             L.ptr(pu8), L.ptr(pi64), L.ptr(tg), L.ptr(confmat), L.ptr(ws), L.stream()), "seg_loss")
    return terms, dl, (pu8 if pu8 is not None else pi64), tg


def softmax_argmax(logits, want="i64", want_maxprob=False):
    B, Cc, H, W = logits.shape
    dev = logits.device
    pu8 = torch.empty(B, H, W, dtype=torch.uint8, device=dev) if want == "u8" else None
    pi64 = torch.empty(B, H, W, dtype=torch.int64, device=dev) if want == "i64" else None
    mp = torch.empty(B, H, W, dtype=torch.float32, device=dev) if want_maxprob else None
    L.check(L.lib().flair_softmax_argmax(L.ptr(logits), B, Cc, H, W, L.ptr(pu8), L.ptr(pi64), L.ptr(mp), L.stream()), "softmax_argmax")
    p = pu8 if pu8 is not None else pi64
    return (p, mp) if want_maxprob else p


def _check_d4(code, H, W):
    code = int(code)
    if not 0 <= code <= 15:
        raise ValueError(f"D4 transform code {code} is outside 0..15 (bit 0 V-flip, bit 1 H-flip, bits 2-3 rot90 count)")
    if code & 4 and H != W:
        raise ValueError(f"D4 transform code {code} has an odd rot90 count: it needs a square tile, not {H} x {W}")
    return code


def d4_transform(x, code):
    """rot90^k(hflip(vflip(x))) of an fp32 (B, C, H, W) tensor for the packed ``code`` (data_feed.pack_d4), out of place"""
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError("d4_transform takes an fp32 (B, C, H, W) tensor")
    B, Cc, H, W = x.shape
    code = _check_d4(code, H, W)
    x = x.contiguous()
    out = torch.empty_like(x)
    L.check(L.lib().flair_d4_nchw_f32(L.ptr(x), L.ptr(out), B, Cc, H, W, code, L.stream()), "flair_d4_nchw_f32")
    return out


def tta_accumulate(logits, code, acc=None, first=False, preds=None, prob=None, n=1, quarter=False):
    """One pass of the test-time-augmentation ensemble (flair_tta_accum / _q4 of include/flair_hip.h): the softmax of ``logits``
    (fp32 (B, C, H, W), or (B, C, H/4, W/4) with ``quarter``), taken in the frame of transform ``code``, goes into ``acc`` (fp32
    (B, C, H, W), stored when ``first`` else added) at the original-frame pixel; with ``preds`` (uint8 (B, H, W)) this is the last
    of ``n`` passes and writes the class and, into ``prob`` (fp32 (B, H, W)), the largest sum / n instead of ``acc``."""
    if logits.dim() != 4 or logits.dtype != torch.float32:
        raise ValueError("tta_accumulate takes fp32 (B, C, h, w) logits")
    B, Cc, h, w = logits.shape
    up = 4 if quarter else 1
    H, W = h * up, w * up
    code = _check_d4(code, H, W)
    if not 1 <= Cc <= 32:
        raise ValueError(f"tta_accumulate takes 1 to 32 classes, not {Cc}")
    if not 1 <= int(n) <= 16:
        raise ValueError(f"tta_accumulate takes 1 to 16 passes, not {n}")
    if quarter and H != W:
        raise ValueError("quarter-resolution logits need a square tile")
    if prob is not None and preds is None:
        raise ValueError("prob needs preds (the last pass writes both)")
    if acc is None and not (first and preds is not None):
        raise ValueError("only a pass that is both first and last runs without acc")
    for t, shape, dt, name in ((acc, (B, Cc, H, W), torch.float32, "acc"), (preds, (B, H, W), torch.uint8, "preds"),
                               (prob, (B, H, W), torch.float32, "prob")):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dt):
            raise ValueError(f"{name} must be {dt} {shape}, got {t.dtype} {tuple(t.shape)}")
    fn = "flair_tta_accum_q4" if quarter else "flair_tta_accum"
    L.check(getattr(L.lib(), fn)(L.ptr(logits), B, Cc, H, W, code, int(bool(first)), L.ptr(acc), L.ptr(preds), L.ptr(prob), int(n),
                                 L.stream()), fn)


def confmat_update(confmat, target, pred):
    Cc = confmat.shape[0]
    L.check(L.lib().flair_confmat_update(L.ptr(target), _LABEL_KIND[target.dtype], L.ptr(pred), _LABEL_KIND[pred.dtype],
                                         target.numel(), Cc, L.ptr(confmat), L.stream()), "confmat_update")
    return confmat


def jaccard(confmat):
    Cc = confmat.shape[0]
    dev = confmat.device
    per = torch.empty(Cc, dtype=torch.float32, device=dev)
    w = torch.empty((), dtype=torch.float32, device=dev)
    m = torch.empty((), dtype=torch.float32, device=dev)
    L.check(L.lib().flair_jaccard(L.ptr(confmat), Cc, L.ptr(per), L.ptr(w), L.ptr(m), L.stream()), "jaccard")
    return per, w, m


def tiff_lzw_slot_bytes(rows_per_strip, W):
    return int(L.lib().flair_tiff_lzw_slot_bytes(int(rows_per_strip), int(W)))


def tiff_lzw_encode(u8, rows_per_strip=None):
    """TIFF 6.0 LZW streams of a (B, H, W) uint8 tensor, one per strip of ``rows_per_strip`` rows (default: libtiff's 8 KB strips).
    Returns (out, counts, slot_bytes, rows_per_strip): strip s of tile b is ``out[b, s, :counts[b, s]]``."""
    if u8.dtype != torch.uint8 or u8.dim() != 3:
        raise L.FlairHipError("tiff_lzw_encode needs a (B, H, W) uint8 tensor")
    B, H, W = u8.shape
    R = max(1, 8192 // W) if rows_per_strip is None else int(rows_per_strip)
    if R < 1:
        raise ValueError(f"rows_per_strip must be at least 1, got {rows_per_strip!r}")
    nstrips = -(-H // R)
    slot = tiff_lzw_slot_bytes(R, W)
    src = L.ptr(u8)   # refuses host and non-contiguous tensors before anything is allocated
    out = torch.empty(B, nstrips, slot, dtype=torch.uint8, device=u8.device)
    counts = torch.empty(B, nstrips, dtype=torch.int32, device=u8.device)
    L.check(L.lib().flair_tiff_lzw_encode(src, B, H, W, R, L.ptr(out), slot, L.ptr(counts), L.stream()), "tiff_lzw_encode")
    return out, counts, slot, R


TIFF_INTERLEAVE = {"band": 0, "pixel": 1}   # PlanarConfiguration 2 / 1 (GDAL's INTERLEAVE=BAND / PIXEL)


def tiff_lzw_tile_slot_bytes(tile, samples):
    return int(L.lib().flair_tiff_lzw_tile_slot_bytes(int(tile), int(samples)))


def tiff_tile_streams(bands, H, W, tile, interleave="band"):
    """how many streams ``tiff_lzw_encode_tiles`` makes of a (bands, H, W) raster"""
    if interleave not in TIFF_INTERLEAVE:
        raise ValueError(f"interleave must be 'band' or 'pixel', got {interleave!r}")
    return (1 if interleave == "pixel" else int(bands)) * -(-int(H) // int(tile)) * -(-int(W) // int(tile))


def tiff_lzw_encode_tiles(raster, tile, interleave="band", scale=None, first_stream=0, n_streams=None):
    """TIFF 6.0 LZW streams of the ``tile`` x ``tile`` TIFF tiles of a (bands, H, W) device raster, uint8 or float32 (include/flair_hip.h:
    the stream order of each ``interleave``, zero padding of edge tiles).  A float32 raster needs ``scale``, one factor per band (a
    sequence or a float32 device tensor): byte = uint8(trunc(min(max(v * scale, 0), 255))), NaN -> 0.  ``first_stream`` / ``n_streams``
    select a window of the streams.  Returns (slots uint8 (n, slot_bytes), counts int32 (n,)): stream first_stream + i is
    ``slots[i, :counts[i]]``."""
    if raster.dim() != 3 or raster.dtype not in (torch.uint8, torch.float32):
        raise L.FlairHipError("tiff_lzw_encode_tiles needs a (bands, H, W) uint8 or float32 tensor")
    bands, H, W = raster.shape
    tile = int(tile)
    if tile < 16 or tile % 16:
        raise ValueError(f"tile must be a positive multiple of 16, got {tile}")
    total = tiff_tile_streams(bands, H, W, tile, interleave)
    f32 = raster.dtype == torch.float32
    if f32 != (scale is not None):
        raise ValueError("a float32 raster needs a scale per band, a uint8 raster takes none")
    src = L.ptr(raster)   # refuses host and non-contiguous tensors before anything is allocated
    if f32:
        if not torch.is_tensor(scale):
            scale = torch.tensor([float(v) for v in scale], dtype=torch.float32).to(raster.device)
        if scale.dtype != torch.float32 or scale.dim() != 1 or scale.numel() != bands:
            raise ValueError(f"scale must hold one float32 factor per band ({bands})")
    first_stream = int(first_stream)
    n = total - first_stream if n_streams is None else int(n_streams)
    if first_stream < 0 or n < 1 or first_stream + n > total:
        raise ValueError(f"streams [{first_stream}, {first_stream + n}) are not a window of the raster's {total}")
    slot = tiff_lzw_tile_slot_bytes(tile, bands if interleave == "pixel" else 1)
    if slot < 0:
        raise ValueError(f"a tile of {tile} x {tile} x {bands} samples is more than one stream holds")
    slots = torch.empty(n, slot, dtype=torch.uint8, device=raster.device)
    counts = torch.empty(n, dtype=torch.int32, device=raster.device)
    L.check(L.lib().flair_tiff_lzw_encode_tiles(src, int(f32), L.ptr(scale), bands, H, W, tile, TIFF_INTERLEAVE[interleave], first_stream, n,
                                                L.ptr(slots), slot, L.ptr(counts), L.stream()), "tiff_lzw_encode_tiles")
    return slots, counts


def tiff_pack_streams(slots, counts, slot_bytes, out=None):
    """Packs encoded streams: (payload, offsets), stream i at ``payload[offsets[i] : offsets[i] + counts[i]]``, every offset a multiple of
    16 (the exclusive sum of the rounded counts, int64 on the device), the bytes between two streams zero.  Without ``out`` the payload is
    a new tensor of exactly the streams' rounded total, which costs one read of that total (a sync); ``out``, a flat uint8 device tensor
    of at least ``n * slot_bytes`` bytes, is packed into without one and returned whole."""
    n = int(counts.numel())
    slot_bytes = int(slot_bytes)
    if n < 1:
        raise ValueError("tiff_pack_streams needs at least one stream")
    if slots.dtype != torch.uint8 or counts.dtype != torch.int32 or slots.numel() != n * slot_bytes:
        raise L.FlairHipError(f"tiff_pack_streams needs uint8 slots of {n} x {slot_bytes} bytes and int32 counts")
    src, cnt = L.ptr(slots), L.ptr(counts)   # refuses host and non-contiguous tensors before anything is allocated
    rounded = (counts.reshape(-1).to(torch.int64) + 15) & ~15
    ends = torch.cumsum(rounded, 0)
    offsets = ends - rounded
    if out is None:
        out = torch.empty(int(ends[-1]), dtype=torch.uint8, device=slots.device)
    elif out.dtype != torch.uint8 or out.dim() != 1 or out.numel() < n * slot_bytes:
        raise L.FlairHipError(f"tiff_pack_streams: out must be a flat uint8 tensor of at least {n * slot_bytes} bytes")
    L.check(L.lib().flair_tiff_pack_streams(src, slot_bytes, cnt, L.ptr(offsets), n, L.ptr(out), out.numel(), L.stream()),
            "tiff_pack_streams")
    return out, offsets


def tiff_lzw_decode_max_strip():
    return int(L.lib().flair_tiff_lzw_decode_max_strip())


_STRIP_TABLE_DTYPES = (("src_off", torch.int64), ("src_len", torch.int32), ("dst_off", torch.int64), ("dst_len", torch.int32),
                       ("mode", torch.int32))


def tiff_lzw_decode(src, src_off, src_len, dst_off, dst_len, mode, dst_bytes, out=None):
    """Decodes TIFF strips on the device: strip i, ``src[src_off[i] : src_off[i] + src_len[i]]``, goes to
    ``dst[dst_off[i] : dst_off[i] + dst_len[i]]``; ``mode[i]`` 0 = stored, 1 = LZW.  ``src`` is a flat uint8 device tensor, the five
    tables are device tensors of one length (offsets int64, the others int32).  Returns (dst uint8 of ``dst_bytes``, status int32 per
    strip; include/flair_hip.h lists the codes).  ``out``, a flat uint8 device tensor of ``dst_bytes``, is decoded into when given."""
    if src.dtype != torch.uint8 or src.dim() != 1:
        raise L.FlairHipError("tiff_lzw_decode needs a flat uint8 tensor of compressed bytes")
    tables = (src_off, src_len, dst_off, dst_len, mode)
    n = int(src_off.numel())
    for t, (name, dt) in zip(tables, _STRIP_TABLE_DTYPES):
        if t.dtype != dt or t.dim() != 1 or t.numel() != n:
            raise L.FlairHipError(f"tiff_lzw_decode: {name} must be a flat {dt} tensor of {n} entries")
    dst_bytes = int(dst_bytes)
    if n < 1 or dst_bytes < 1:
        raise ValueError("tiff_lzw_decode needs at least one strip and dst_bytes >= 1")
    ptrs = [L.ptr(src)] + [L.ptr(t) for t in tables]   # refuses host and non-contiguous tensors before anything is allocated
    if out is None:
        out = torch.empty(dst_bytes, dtype=torch.uint8, device=src.device)
    elif out.dtype != torch.uint8 or out.dim() != 1 or out.numel() != dst_bytes:
        raise L.FlairHipError(f"tiff_lzw_decode: out must be a flat uint8 tensor of {dst_bytes} bytes")
    status = torch.empty(n, dtype=torch.int32, device=src.device)
    L.check(L.lib().flair_tiff_lzw_decode(ptrs[0], src.numel(), *ptrs[1:], n, L.ptr(out), dst_bytes, L.ptr(status), L.stream()),
            "tiff_lzw_decode")
    return out, status


def tiff_lzw_decode_chunks_cap():
    return int(L.lib().flair_tiff_lzw_decode_chunks_cap())


def tiff_lzw_decode_chunks_window():
    return int(L.lib().flair_tiff_lzw_decode_chunks_window())


TIFF_SLOT_ALIGN = 128   # slots of tiff_lzw_decode_chunks: the base and slot_bytes are multiples of it

_CHUNK_TABLE_DTYPES = (("src_off", torch.int64), ("src_len", torch.int32), ("dst_len", torch.int32), ("mode", torch.int32))


def tiff_lzw_decode_chunks(src, src_off, src_len, dst_len, mode, slot_bytes, out=None, status=None):
    """Decodes the chunks (tiles or strips) of a TIFF on the device: chunk i, ``src[src_off[i] : src_off[i] + src_len[i]]``, goes to
    ``scratch[i, :dst_len[i]]``; ``mode[i]`` 0 = stored, 1 = LZW, decoded lengths up to ``tiff_lzw_decode_chunks_cap()``.  ``src`` is a
    flat uint8 device tensor, the four tables are device tensors of one length (offsets int64, the others int32), ``slot_bytes`` a
    multiple of 128.  Returns (scratch uint8 (n, slot_bytes), status int32 per chunk; include/flair_hip.h lists the codes).  ``out``, a
    uint8 device tensor of n * slot_bytes bytes whose address is a multiple of 128, is decoded into when given, and ``status``, a flat int32
    device tensor of n entries, receives the codes."""
    if src.dtype != torch.uint8 or src.dim() != 1:
        raise L.FlairHipError("tiff_lzw_decode_chunks needs a flat uint8 tensor of compressed bytes")
    tables = (src_off, src_len, dst_len, mode)
    n = int(src_off.numel())
    for t, (name, dt) in zip(tables, _CHUNK_TABLE_DTYPES):
        if t.dtype != dt or t.dim() != 1 or t.numel() != n:
            raise L.FlairHipError(f"tiff_lzw_decode_chunks: {name} must be a flat {dt} tensor of {n} entries")
    slot_bytes = int(slot_bytes)
    if n < 1 or slot_bytes < TIFF_SLOT_ALIGN or slot_bytes % TIFF_SLOT_ALIGN:
        raise ValueError(f"tiff_lzw_decode_chunks needs at least one chunk and slot_bytes a positive multiple of {TIFF_SLOT_ALIGN}")
    ptrs = [L.ptr(src)] + [L.ptr(t) for t in tables]   # refuses host and non-contiguous tensors before anything is allocated
    if out is None:
        out = torch.empty(n, slot_bytes, dtype=torch.uint8, device=src.device)
    elif out.dtype != torch.uint8 or out.numel() != n * slot_bytes or out.data_ptr() % TIFF_SLOT_ALIGN:
        raise L.FlairHipError(f"tiff_lzw_decode_chunks: out must be a uint8 tensor of {n} x {slot_bytes} bytes at a multiple of "
                              f"{TIFF_SLOT_ALIGN}")
    if status is None:
        status = torch.empty(n, dtype=torch.int32, device=src.device)
    elif status.dtype != torch.int32 or status.dim() != 1 or status.numel() != n:
        raise L.FlairHipError(f"tiff_lzw_decode_chunks: status must be a flat int32 tensor of {n} entries")
    L.check(L.lib().flair_tiff_lzw_decode_chunks(ptrs[0], src.numel(), *ptrs[1:], n, L.ptr(out), slot_bytes, L.ptr(status), L.stream()),
            "tiff_lzw_decode_chunks")
    return out.view(n, slot_bytes), status


def tiff_chunks_to_planes(scratch, chunks, status, planes, samples, predictor=1, max_rows=None):
    """Scatters decoded chunks into the (bands, H, W) uint8 device raster ``planes``, in place: ``scratch`` (n, slot_bytes) uint8 as
    ``tiff_lzw_decode_chunks`` returns it, ``chunks`` (n, 5) int32 rows {x0, y0, width, rows, band0} on the device, ``status`` int32 per
    chunk (chunks whose status is not 0 are skipped).  ``samples`` bytes per pixel of a slot: 1 or bands; ``predictor`` 1 or 2 (TIFF
    horizontal differencing, undone per chunk row and sample).  ``max_rows``: the largest ``rows`` of the table when the caller knows
    it; otherwise it is read from the device, which waits for it.  Returns ``planes``."""
    if scratch.dtype != torch.uint8 or scratch.dim() != 2:
        raise L.FlairHipError("tiff_chunks_to_planes needs the (n, slot_bytes) uint8 scratch of tiff_lzw_decode_chunks")
    n, slot_bytes = scratch.shape
    if chunks.dtype != torch.int32 or tuple(chunks.shape) != (n, 5) or status.dtype != torch.int32 or tuple(status.shape) != (n,):
        raise L.FlairHipError(f"tiff_chunks_to_planes: chunks must be ({n}, 5) int32 and status ({n},) int32")
    if planes.dtype != torch.uint8 or planes.dim() != 3:
        raise L.FlairHipError("tiff_chunks_to_planes writes a (bands, H, W) uint8 raster")
    bands, H, W = planes.shape
    samples, predictor = int(samples), int(predictor)
    if samples not in (1, bands):
        raise ValueError(f"samples must be 1 or the raster's {bands} bands, got {samples}")
    if predictor not in (1, 2):
        raise ValueError(f"predictor must be 1 or 2, got {predictor}")
    ptrs = [L.ptr(scratch), L.ptr(chunks), L.ptr(status), L.ptr(planes)]
    if max_rows is None:
        max_rows = int(chunks[:, 3].max())
    L.check(L.lib().flair_tiff_chunks_to_planes(ptrs[0], slot_bytes, ptrs[1], ptrs[2], n, max(1, int(max_rows)), samples, predictor,
                                                ptrs[3], bands, H, W, L.stream()), "tiff_chunks_to_planes")
    return planes


def tiff_chunks_to_batch(scratch, chunks, status, planes, max_rows=None):
    """Scatters the decoded chunks of a batch of files into ``planes``, a uint8 device tensor whose last two axes are (H, W) and whose
    leading axes count the planes ((B, bands, H, W) images, (B, H, W) masks), in place: ``scratch`` (n, slot_bytes) uint8 as
    ``tiff_lzw_decode_chunks`` returns it, ``chunks`` (n, 8) int32 rows {x0, y0, width, rows, plane0, samples, predictor, 0} on the
    device, ``status`` int32 per chunk (chunks whose status is not 0 are skipped).  Samples and predictor are per chunk: the files of
    a batch may differ in layout.  ``max_rows``: the largest ``rows`` of the table when the caller knows it; otherwise it is read from
    the device, which waits for it.  Returns ``planes``."""
    if scratch.dtype != torch.uint8 or scratch.dim() != 2:
        raise L.FlairHipError("tiff_chunks_to_batch needs the (n, slot_bytes) uint8 scratch of tiff_lzw_decode_chunks")
    n, slot_bytes = scratch.shape
    if chunks.dtype != torch.int32 or tuple(chunks.shape) != (n, 8) or status.dtype != torch.int32 or tuple(status.shape) != (n,):
        raise L.FlairHipError(f"tiff_chunks_to_batch: chunks must be ({n}, 8) int32 and status ({n},) int32")
    if planes.dtype != torch.uint8 or planes.dim() < 3:
        raise L.FlairHipError("tiff_chunks_to_batch writes a (..., H, W) uint8 tensor of planes")
    H, W = planes.shape[-2:]
    n_planes = planes.numel() // max(1, H * W)
    ptrs = [L.ptr(scratch), L.ptr(chunks), L.ptr(status), L.ptr(planes)]
    if max_rows is None:
        max_rows = int(chunks[:, 3].max())
    L.check(L.lib().flair_tiff_chunks_to_batch(ptrs[0], slot_bytes, ptrs[1], ptrs[2], n, max(1, int(max_rows)), ptrs[3], n_planes, H, W,
                                               L.stream()), "tiff_chunks_to_batch")
    return planes


def sgd_step_(params_flat, grads_flat, lr):
    L.check(L.lib().flair_sgd_step(L.ptr(params_flat), L.ptr(grads_flat), params_flat.numel(), float(lr), L.stream()), "sgd_step")


# ---- update rules over flat fp32 buffers (flair_optim_* / flair_grad_sqnorm / flair_clip_coef of include/flair_hip.h)
def _check_flat_f32(n, **tensors):
    for name, t in tensors.items():
        if t is not None and (t.dim() != 1 or t.dtype != torch.float32 or t.numel() != n):
            raise ValueError(f"{name} must be fp32 ({n},), got {t.dtype} {tuple(t.shape)}")


def _check_coef(coef):
    if coef is not None and (coef.dtype != torch.float32 or coef.numel() != 1):
        raise ValueError("coef must be one fp32 device value")


def optim_sgd_(params, grads, buf, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, first=False, grad_scale=1.0,
               coef=None):
    """torch.optim.SGD's rule on flat buffers, in place on ``params`` and ``buf`` (the momentum buffer; None without momentum):
    g' = grads * grad_scale * coef, then weight decay, momentum (``first``: buf = g', its content unread), nesterov, p -= lr g'."""
    if params.dim() != 1 or params.dtype != torch.float32:
        raise ValueError("optim_sgd_ takes flat fp32 buffers")
    n = params.numel()
    _check_flat_f32(n, grads=grads, buf=buf)
    _check_coef(coef)
    if momentum != 0 and buf is None:
        raise ValueError("momentum needs its buffer")
    if nesterov and (momentum <= 0 or dampening != 0):
        raise ValueError("Nesterov momentum requires a momentum and zero dampening")
    L.check(L.lib().flair_optim_sgd(L.ptr(params), L.ptr(grads), L.ptr(buf), n, float(lr), float(momentum), float(dampening),
                                    float(weight_decay), int(bool(nesterov)), int(bool(first)), float(grad_scale), L.ptr(coef),
                                    L.stream()), "optim_sgd")


def adamw_bias_corrections(betas, step):
    """(1 - beta1^t, 1 - beta2^t) in fp64, as the host hands them to flair_optim_adamw"""
    return 1.0 - float(betas[0]) ** int(step), 1.0 - float(betas[1]) ** int(step)


def optim_adamw_(params, grads, exp_avg, exp_avg_sq, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, step=1, first=False,
                 grad_scale=1.0, coef=None):
    """torch.optim.AdamW's rule on flat buffers, in place on ``params``, ``exp_avg`` and ``exp_avg_sq``; ``step`` is t of the bias
    corrections (1-based), ``first`` takes both moments as zero whatever the buffers hold."""
    if params.dim() != 1 or params.dtype != torch.float32:
        raise ValueError("optim_adamw_ takes flat fp32 buffers")
    n = params.numel()
    _check_flat_f32(n, grads=grads, exp_avg=exp_avg, exp_avg_sq=exp_avg_sq)
    _check_coef(coef)
    if exp_avg is None or exp_avg_sq is None:
        raise ValueError("AdamW needs both moment buffers")
    if int(step) < 1:
        raise ValueError(f"step counts from 1, got {step}")
    bc1, bc2 = adamw_bias_corrections(betas, step)
    L.check(L.lib().flair_optim_adamw(L.ptr(params), L.ptr(grads), L.ptr(exp_avg), L.ptr(exp_avg_sq), n, float(lr), float(betas[0]),
                                      float(betas[1]), float(eps), float(weight_decay), bc1, bc2, int(bool(first)), float(grad_scale),
                                      L.ptr(coef), L.stream()), "optim_adamw")


def grad_sqnorm_partials():
    return int(L.lib().flair_grad_sqnorm_partials())


def grad_sqnorm_(grads, sq_sum, partials, accumulate=False):
    """sq_sum (one fp64 device value) = (its content if ``accumulate`` else 0) + sum of grads^2; ``partials``: fp64 workspace of
    grad_sqnorm_partials() elements.  Fixed summation order: the same bits on every run."""
    if grads.dim() != 1 or grads.dtype != torch.float32:
        raise ValueError("grad_sqnorm_ takes a flat fp32 buffer")
    if sq_sum.dtype != torch.float64 or sq_sum.numel() != 1:
        raise ValueError("sq_sum must be one fp64 device value")
    if partials.dtype != torch.float64 or partials.numel() < grad_sqnorm_partials():
        raise ValueError(f"partials must hold {grad_sqnorm_partials()} fp64 values")
    L.check(L.lib().flair_grad_sqnorm(L.ptr(grads), grads.numel(), L.ptr(partials), L.ptr(sq_sum), int(bool(accumulate)), L.stream()),
            "grad_sqnorm")
    return sq_sum


def clip_coef_(sq_sum, max_norm, norm, coef, grad_scale=1.0):
    """clip_grad_norm_'s rule from the fp64 sum of squares: norm = sqrt(sq_sum) * grad_scale, coef = min(1, max_norm / (norm + 1e-6)),
    both written as fp32 device values; nothing comes back to the host."""
    if sq_sum.dtype != torch.float64 or sq_sum.numel() != 1:
        raise ValueError("sq_sum must be one fp64 device value")
    for name, t in (("norm", norm), ("coef", coef)):
        if t.dtype != torch.float32 or t.numel() != 1:
            raise ValueError(f"{name} must be one fp32 device value")
    if not float(max_norm) > 0:
        raise ValueError(f"max_norm must be positive, got {max_norm}")
    L.check(L.lib().flair_clip_coef(L.ptr(sq_sum), float(grad_scale), float(max_norm), L.ptr(norm), L.ptr(coef), L.stream()), "clip_coef")


# ---- the SegFormer / UperNet-Swin kernels one at a time (the launchers the two executors call).  `rc=True` returns the
# launcher's return code instead of raising, so that a refusal (-2) can be asserted.
def _ret(rc, what, out, want_rc):
    if want_rc:
        return rc
    L.check(rc, what)
    return out


def _bf16(t):
    return t.to(torch.bfloat16).contiguous()


def sf_layernorm(x, gamma, beta, eps, rc=False):
    C = x.shape[-1]
    y = torch.empty_like(x)
    return _ret(L.lib().flair_sf_layernorm(_dt(x), L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(y), x.numel() // C, C, float(eps),
                                           L.stream()), "sf_layernorm", y, rc)


def swin_layernorm(x, gamma, beta, eps, out=None, rc=False):
    """out (optional): rows of ld = out.shape[-1] >= C elements, columns [0, C) written."""
    C = x.shape[-1]
    y = torch.empty_like(x) if out is None else out
    return _ret(L.lib().flair_swin_layernorm(_dt(x), L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(y), x.numel() // C, C, y.shape[-1],
                                             float(eps), L.stream()), "swin_layernorm", y, rc)


def swin_patch_merge_ln(x, gamma, beta, eps, rc=False):
    B, H, W, C = x.shape
    y = torch.empty(B, H // 2, W // 2, 4 * C, dtype=x.dtype, device=x.device)
    return _ret(L.lib().flair_swin_patch_merge_ln(_dt(x), L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(y), B, H, W, C, float(eps),
                                                  L.stream()), "swin_patch_merge_ln", y, rc)


def sf_dwconv3x3_gelu(x, w, bias, rc=False):
    """x [B][H][W][C], w [C][3][3] (or [C][1][3][3]) fp32, bias [C] fp32"""
    B, H, W, C = x.shape
    y = torch.empty_like(x)
    return _ret(L.lib().flair_sf_dwconv3x3_gelu(_dt(x), L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(y), B, H, W, C, L.stream()),
                "sf_dwconv3x3_gelu", y, rc)


def sf_bilinear_nhwc(x, H, W, out=None, rc=False):
    """out (optional) [B][H][W][ld >= C]: channels [0, C) written"""
    B, h, w, C = x.shape
    y = torch.empty(B, H, W, C, dtype=x.dtype, device=x.device) if out is None else out
    return _ret(L.lib().flair_sf_bilinear_nhwc(_dt(x), L.ptr(x), L.ptr(y), B, h, w, C, H, W, y.shape[-1], L.stream()),
                "sf_bilinear_nhwc", y, rc)


def sf_bilinear_nchw_f32(x, H, W, rc=False):
    B, Cc, h, w = x.shape
    y = torch.empty(B, Cc, H, W, dtype=torch.float32, device=x.device)
    return _ret(L.lib().flair_sf_bilinear_nchw_f32(L.ptr(x), L.ptr(y), B * Cc, h, w, H, W, L.stream()), "sf_bilinear_nchw_f32", y, rc)


def sf_slice_cols(src, col0, ncols, dtype, rc=False):
    """fp32 [rows][ld] columns [col0, col0 + ncols) -> dtype [rows][ncols]"""
    rows, ld = src.shape
    dt = L.dtype_code(dtype)
    y = torch.empty(rows, ncols, dtype=L.torch_dtype(dt), device=src.device)
    return _ret(L.lib().flair_sf_slice_cols(dt, L.ptr(src), ld, col0, ncols, rows, L.ptr(y), L.stream()), "sf_slice_cols", y, rc)


def sf_fuse_bias(wf, b3, b2, b1, b0, scale, shift, rc=False):
    D = wf.shape[0]
    y = torch.empty(D, dtype=torch.float32, device=wf.device)
    return _ret(L.lib().flair_sf_fuse_bias(L.ptr(wf), D, L.ptr(b3), L.ptr(b2), L.ptr(b1), L.ptr(b0), L.ptr(scale), L.ptr(shift),
                                           L.ptr(y), L.stream()), "sf_fuse_bias", y, rc)


def sf_upsample_sum_bn_relu(g0, g1, g2, g3, scale, shift2, rc=False):
    B, H, W, D = g0.shape
    z = torch.empty_like(g0)
    return _ret(L.lib().flair_sf_upsample_sum_bn_relu(_dt(g0), L.ptr(g0), L.ptr(g1), L.ptr(g2), L.ptr(g3), L.ptr(scale), L.ptr(shift2),
                                                      L.ptr(z), B, H, W, D, L.stream()), "sf_upsample_sum_bn_relu", z, rc)


def sf_ffn_fused_ok(dtype, C, H, W):
    return bool(L.lib().flair_sf_ffn_fused_ok(L.dtype_code(dtype), C, H, W))


def sf_ffn_fused(x, ln_g, ln_b, w1, b1, dw_w, dw_b, w2, b2, eps, ln2_g=None, ln2_b=None, want_ln=False, out=None, out_ln=None,
                 rc=False):
    """x bf16 [B][H][W][C]; w1 [4C][C], w2 [C][4C], dw_w [4C][3][3] fp32 (the two matrices are packed to bf16 row-major here).
    Returns (out, out_ln)."""
    B, H, W, C = x.shape
    l = L.lib()
    dwp = sf_ffn_dw_pack(dw_w, dw_b)
    w1p, w2p = _bf16(w1), _bf16(w2)
    out = torch.empty_like(x) if out is None else out
    if want_ln and out_ln is None:
        out_ln = torch.empty_like(x)
    r = l.flair_sf_ffn_fused(L.ptr(x), L.ptr(ln_g), L.ptr(ln_b), L.ptr(w1p), L.ptr(b1), L.ptr(dwp), L.ptr(w2p), L.ptr(b2), L.ptr(out),
                             B, H, W, C, float(eps), L.ptr(ln2_g), L.ptr(ln2_b), L.ptr(out_ln), L.stream())
    return _ret(r, "sf_ffn_fused", (out, out_ln), rc)


def sf_ffn_dw_pack(dw_w, dw_b):
    nch = dw_b.numel()
    dwp = torch.empty(nch // 4, 10, 4, dtype=torch.float32, device=dw_w.device)
    dw_w = dw_w.contiguous()
    L.check(L.lib().flair_sf_ffn_dw_pack(L.ptr(dw_w), L.ptr(dw_b), L.ptr(dwp), nch, L.stream()), "sf_ffn_dw_pack")
    return dwp


def sf_head_fused_ok(dtype, H, W, C0, D, labels):
    return bool(L.lib().flair_sf_head_fused_ok(L.dtype_code(dtype), H, W, C0, D, labels))


def sf_head_wint(device):
    w = torch.empty(128, 96, dtype=torch.bfloat16, device=device)
    L.check(L.lib().flair_sf_head_wint(L.ptr(w), L.stream()), "sf_head_wint")
    return w


def sf_head_fused(f0, w0, g1, g2, g3, scale, shift2, wc, bc, rc=False):
    """f0 bf16 [B][H][W][64], g_i bf16 [B][H >> i][W >> i][D]; w0 [D][64], wc [labels][D] fp32 (packed to bf16 here, wc padded to
    32 rows of zeros); logits fp32 NCHW"""
    B, H, W, _ = f0.shape
    D, labels = w0.shape[0], wc.shape[0]
    wcp = torch.zeros(32, D, dtype=torch.bfloat16, device=f0.device)
    wcp[:min(labels, 32)] = wc[:32].to(torch.bfloat16)
    out = torch.empty(B, labels, H, W, dtype=torch.float32, device=f0.device)
    w0p, wint = _bf16(w0), sf_head_wint(f0.device)   # named: a temporary's block would be handed to the next allocation
    r = L.lib().flair_sf_head_fused(L.ptr(f0), L.ptr(w0p), L.ptr(g1), L.ptr(g2), L.ptr(g3), L.ptr(wint),
                                    L.ptr(scale), L.ptr(shift2), L.ptr(wcp), L.ptr(bc), L.ptr(out), B, H, W, D, labels, L.stream())
    return _ret(r, "sf_head_fused", out, rc)


def sf_attention(q, k, v, kv_ld=None, rc=False):
    """q [B][N][hidden]; k, v [B][Nk] rows of kv_ld elements (views into one [B][Nk][2 * hidden] buffer allowed: pass kv_ld)"""
    B, N, hidden = q.shape
    Nk = k.shape[1]
    kv_ld = kv_ld or k.shape[2]
    out = torch.empty_like(q)
    r = L.lib().flair_sf_attention(_dt(q), L.ptr(q), k.data_ptr(), v.data_ptr(), L.ptr(out), B, N, Nk, hidden, kv_ld, L.stream())
    return _ret(r, "sf_attention", out, rc)


def swin_window_attention(qkv, qkv_bias, table, heads, shift, rc=False):
    """qkv [B][H][W][3C] (biases included), qkv_bias [3C], table [169][heads] fp32 -> [B][H][W][C]"""
    B, H, W, C3 = qkv.shape
    out = torch.empty(B, H, W, C3 // 3, dtype=qkv.dtype, device=qkv.device)
    r = L.lib().flair_swin_window_attention(_dt(qkv), L.ptr(qkv), L.ptr(qkv_bias), L.ptr(table), L.ptr(out), B, H, W, C3 // 3, heads,
                                            shift, L.stream())
    return _ret(r, "swin_window_attention", out, rc)


def swin_adaptive_avgpool(x, C, S, rc=False):
    """x [B][h][w][ld >= C] -> [B][S][S][C]"""
    B, h, w, ld = x.shape
    y = torch.empty(B, S, S, C, dtype=x.dtype, device=x.device)
    return _ret(L.lib().flair_swin_adaptive_avgpool(_dt(x), L.ptr(x), ld, L.ptr(y), B, h, w, C, S, L.stream()), "swin_adaptive_avgpool",
                y, rc)


def swin_bilinear_add_(y, x, rc=False):
    """y [B][H][W][C] += bilinear(x [B][h][w][C]) in place"""
    B, H, W, C = y.shape
    _, h, w, _ = x.shape
    return _ret(L.lib().flair_swin_bilinear_add(_dt(x), L.ptr(x), L.ptr(y), B, h, w, C, H, W, L.stream()), "swin_bilinear_add", y, rc)
