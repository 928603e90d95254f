"""Case table, references and bounds of the configurable-loss head's tests (csrc/seg_loss.hip: test_gpu_seg_loss.py,
test_seg_loss_cases_cpu.py).  Inputs are those of the cross-entropy head's tests (ce_head_cases: logits of the ``ints`` and ``far``
families, the four label kinds with their ignored values, the three weight settings); this module adds

* ``reference_of``: the definitions of flair_amd/losses.py in fp64 torch with autograd;
* ``dice_gradient_closed_form``: the Dice gradient as the kernels form it (per-class pair, p_k (g_k - sum_c g_c p_c)), in fp64;
* ``kernel_arithmetic_f32``: the kernels' arithmetic restated in fp32 on the CPU, operation by operation;
* ``CASES``: a pairwise table over C, shape, logit family, weights, label kind, row stride and specification;
* the bounds: the project's own for this arithmetic (ce_head_cases.loss_bound for the loss and both terms, ce_head_cases.dl_bound
  for the gradient); the fp32 restatement keeps them with 4x to spare for every specification of the table (see below).

This module needs no device."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import torch
import torch.nn.functional as F

import ce_head_cases as K

SMALL, MEDIUM, LARGE = K.SMALL, K.MEDIUM, K.LARGE

# name -> SegLoss arguments
SPECS = {
    "ls": dict(label_smoothing=0.1),
    "focal2": dict(focal_gamma=2.0),
    "focal15": dict(focal_gamma=1.5),
    "dice": dict(ce=0.0, dice=1.0),
    "dice_s1": dict(ce=0.0, dice=1.0, dice_smooth=1.0),
    "ce_dice_ls": dict(ce=1.0, dice=1.0, label_smoothing=0.1),
}

# The restatement was measured against the fp64 reference over CASES (test_seg_loss_cases_cpu.py prints every figure): relative to
# max |dl| its largest gradient error is 2.3e-7 with label smoothing, 5.4e-7 with Dice and 1.7e-6 with a focal term (focal2, C = 19,
# LARGE; 3.6e-7 at C = 13 in the ``far`` family, where nll reaches 240) -- every specification keeps the CE head's bounds with 4x to
# spare, the focal ones because q is summed from the other classes and the label's column is -q.  So no specification has a bound of
# its own: loss_bound and dl_bound are ce_head_cases'.


def spec_of(name):
    from flair_amd.losses import SegLoss
    return SegLoss(**SPECS[name])


def loss_bound(ref):
    return K.loss_bound(ref)


def dl_bound(ref_dl):
    return K.dl_bound(ref_dl)


@dataclass(frozen=True)
class SegCase:
    C: int
    ld: int          # row stride of the NHWC runs
    shape: tuple
    family: str      # ints | far
    weight: str      # none | rand | zeros
    kind: str        # u8 | i32 | i64 | onehot
    spec: str        # key of SPECS

    @property
    def name(self):
        return f"c{self.C}_ld{self.ld}_{'x'.join(map(str, self.shape))}_{self.family}_{self.weight}_{self.kind}_{self.spec}"

    @property
    def values(self):
        return self.C, self.shape, self.family, self.weight

    @property
    def npix(self):
        return self.shape[0] * self.shape[1] * self.shape[2]


CASES = [
    SegCase(13, 16, SMALL, "ints", "none", "u8", "ls"),
    SegCase(19, 32, MEDIUM, "far", "rand", "i32", "ls"),
    SegCase(32, 32, SMALL, "far", "rand", "i64", "ls"),
    SegCase(2, 16, MEDIUM, "ints", "rand", "i64", "focal2"),
    SegCase(13, 32, SMALL, "far", "none", "onehot", "focal2"),
    SegCase(13, 16, MEDIUM, "far", "rand", "u8", "focal2"),
    SegCase(19, 32, MEDIUM, "far", "zeros", "u8", "focal15"),
    SegCase(32, 32, SMALL, "ints", "rand", "i32", "focal15"),
    SegCase(13, 16, MEDIUM, "far", "rand", "i64", "dice"),
    SegCase(19, 32, SMALL, "ints", "zeros", "onehot", "dice"),
    SegCase(32, 32, MEDIUM, "far", "none", "u8", "dice_s1"),
    SegCase(2, 16, SMALL, "ints", "none", "i32", "dice_s1"),
    SegCase(13, 16, MEDIUM, "ints", "rand", "onehot", "ce_dice_ls"),
    SegCase(19, 32, MEDIUM, "far", "zeros", "i64", "ce_dice_ls"),
    SegCase(2, 32, SMALL, "far", "rand", "u8", "ce_dice_ls"),
    # past the grid cap: the only large cases
    SegCase(13, 16, LARGE, "far", "rand", "i64", "ce_dice_ls"),
    SegCase(19, 32, LARGE, "ints", "zeros", "u8", "focal2"),
]


def labels_and_valid(lab, kind):
    """(y int64, valid bool) as the kernels read the labels of a kind."""
    if kind == "onehot":
        return lab["y_onehot"], torch.ones_like(lab["ign"])
    return lab["y"], ~lab["ign"]


# ------------------------------------------------------------------------------------------------ fp64 reference
def terms_torch(xd, y, valid, w, spec):
    """(CE, Dice) of flair_amd/losses.py in plain torch operations, in the dtype and on the device of the logits ``xd`` (fp64 for the
    reference; the trainer tests' twins step through it in fp32 on the device)."""
    C = xd.shape[1]
    f64 = xd.dtype
    wv = torch.ones(C, dtype=f64, device=xd.device) if w is None else w.to(device=xd.device, dtype=f64)
    logp = torch.log_softmax(xd, 1)
    p = logp.exp()
    yy = torch.where(valid, y, torch.zeros_like(y))
    vf = valid.to(f64)
    oh = F.one_hot(yy, C).permute(0, 3, 1, 2).to(f64) * vf[:, None]
    wy = wv[yy] * vf
    D = wy.sum()
    nll = -(logp * oh).sum(1)
    ce = torch.zeros((), dtype=f64, device=xd.device)
    if spec.ce > 0:
        if spec.focal_gamma == 0:
            e = spec.label_smoothing
            allc = -(logp * wv[None, :, None, None]).sum(1) * vf
            ce = ((1 - e) * wy * nll + (e / C) * allc).sum() / D
        else:
            q = (p * (1 - oh)).sum(1)          # summed from the other classes
            ce = (wy * q ** spec.focal_gamma * nll).sum() / D
    dice = torch.zeros((), dtype=f64, device=xd.device)
    if spec.dice > 0:
        kf = (valid & (wv[yy] > 0)).to(f64)[:, None]
        I = (p * oh * kf).sum((0, 2, 3))
        P = (p * kf).sum((0, 2, 3))
        T = (oh * kf).sum((0, 2, 3))
        s = spec.dice_smooth
        dice = ((T > 0).to(f64) * (1 - (2 * I + s) / torch.clamp_min(P + T + s, spec.dice_eps))).sum() / C
    return ce, dice


def reference_of(x, y, valid, w, spec):
    """loss = ce * CE + dice * Dice of flair_amd/losses.py in fp64 with autograd: dict loss, ce, dice (floats), dl (B, C, H, W)."""
    xd = x.double().requires_grad_(True)
    ce, dice = terms_torch(xd, y, valid, w, spec)
    loss = spec.ce * ce + spec.dice * dice
    if loss.requires_grad:
        (dl,) = torch.autograd.grad(loss, xd)
    else:
        dl = torch.zeros_like(xd)       # no counted pixel and no CE term: a constant
    return {"loss": float(loss.detach()), "ce": float(ce.detach()), "dice": float(dice.detach()), "dl": dl.detach()}


def dice_gradient_closed_form(x, y, valid, w, spec):
    """d (dice * Dice) / dz in fp64 by the formula the kernels use: the per-class pair (g_c for y != c, g_c for y == c) from the
    sums, then k p_k (g_k - sum_c g_c p_c)."""
    C = x.shape[1]
    f64 = torch.float64
    wv = torch.ones(C, dtype=f64) if w is None else w.to(f64)
    p = torch.softmax(x.double(), 1)
    yy = torch.where(valid, y, torch.zeros_like(y))
    k = valid & (wv[yy] > 0)
    oh = F.one_hot(yy, C).permute(0, 3, 1, 2).to(f64) * k.to(f64)[:, None]
    kf = k.to(f64)[:, None]
    I, P, T = (p * oh).sum((0, 2, 3)), (p * kf).sum((0, 2, 3)), oh.sum((0, 2, 3))
    s = spec.dice_smooth
    den = P + T + s
    assert bool((den[T > 0] >= spec.dice_eps).all()), "the clamp is active: the closed form below is the unclamped one"
    present = (T > 0).to(f64) / C
    den = torch.where(T > 0, den, torch.ones_like(den))
    gno = present * (2 * I + s) / den ** 2
    gyes = gno - present * 2 / den
    g = gno[None, :, None, None] * (1 - oh) + gyes[None, :, None, None] * oh
    dot = (g * p).sum(1, keepdim=True)
    return spec.dice * kf * p * (g - dot)


@functools.lru_cache(maxsize=4)
def case_reference(case):
    """(inputs of the case's values, y, valid, fp64 reference)."""
    v = K.case_values(*case.values)
    y, valid = labels_and_valid(v["lab"], case.kind)
    return v, y, valid, reference_of(v["x"], y, valid, v["w"], spec_of(case.spec))


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic in fp32
def _block_partials(vals):
    """fp32 sums over runs of 256 pixels, their sum in fp64 (block partials, then the one-block fp64 sum)."""
    f32 = torch.float32
    pad = (-vals.shape[0]) % 256
    v = torch.cat([vals.to(f32), torch.zeros((pad,) + vals.shape[1:], dtype=f32)])
    return v.view(-1, 256, *vals.shape[1:]).sum(1, dtype=f32).double().sum(0)


def kernel_arithmetic_f32(x, y, valid, w, spec):
    """seg_loss.hip restated in fp32: max, exp(x - m), the sum in class order, p = e * (1 / sum); the CE contribution per term set
    (plain / smoothed through sum_c w[c] (z_c - m) and log(sum e) / focal with q summed from the other classes and -q in the label's
    column); the Dice sums in fp32 block partials and fp64, the per-class gradient pair rounded to fp32, p_k (g_k - sum_c g_c p_c).
    Returns dict loss, ce, dice (floats, as the fp32 outputs hold them), dl (B, C, H, W) fp32, preds."""
    B, C, H, W = x.shape
    f32 = torch.float32
    rows = x.permute(0, 2, 3, 1).reshape(-1, C).to(f32)
    npix = rows.shape[0]
    yy = torch.where(valid, y, torch.zeros_like(y)).reshape(-1)
    ok = valid.reshape(-1)
    okf = ok.to(f32)
    wv = (torch.ones(C) if w is None else w).to(f32)
    m = rows.max(1).values
    e = torch.exp(rows - m[:, None])
    s = torch.zeros_like(m)
    for c in range(C):
        s = s + e[:, c]
    p = e * (1.0 / s)[:, None]
    preds = p.argmax(1)
    wy = wv[yy] * okf
    xy = rows.gather(1, yy[:, None])[:, 0]
    onehot = torch.zeros_like(rows)
    onehot[torch.arange(npix), yy] = okf
    lse = torch.log(s)
    nll = lse - (xy - m)
    den = _block_partials(wy).to(f32)
    g = torch.zeros_like(rows)
    ce = 0.0
    if spec.ce > 0:
        cscale = torch.tensor(spec.ce, dtype=f32) * (1.0 / den)
        if spec.focal_gamma > 0:
            gam = torch.tensor(spec.focal_gamma, dtype=f32)
            q = torch.zeros_like(m)
            for c in range(C):
                q = q + torch.where(ok & (yy == c), torch.zeros_like(m), p[:, c])
            py = p.gather(1, yy[:, None])[:, 0] * okf
            qg1 = torch.pow(q, gam - 1.0)
            term = wy * (qg1 * q) * nll
            sc = wy * (qg1 * (gam * nll * py + q)) * cscale
            g = torch.where(onehot.bool(), -q[:, None].expand_as(p), p) * sc[:, None]
        elif spec.label_smoothing > 0:
            keep = torch.tensor(1.0, dtype=f32) - torch.tensor(spec.label_smoothing, dtype=f32)
            lsc = torch.tensor(spec.label_smoothing, dtype=f32) / torch.tensor(float(C), dtype=f32)
            wsum = torch.zeros((), dtype=f32)
            swz = torch.zeros_like(m)
            for c in range(C):
                wsum = wsum + wv[c]
                swz = swz + wv[c] * (rows[:, c] - m)
            term = (keep * wy * nll + lsc * (wsum * lse - swz)) * okf
            ga = (keep * wy + lsc * wsum) * cscale * okf
            gy = keep * wy * cscale
            gs = lsc * cscale * okf
            g = p * ga[:, None] - onehot * gy[:, None] - wv[None, :] * gs[:, None]
        else:
            term = wy * nll
            g = (p - onehot) * (wy * cscale)[:, None]
        ce = float((_block_partials(term * okf) / den.double()).to(f32))
    dice = 0.0
    if spec.dice > 0:
        k = ok & (wy > 0)
        kf = k.to(f32)
        I = _block_partials(p * onehot * kf[:, None])
        P = _block_partials(p * kf[:, None])
        T = (onehot * kf[:, None]).double().sum(0)
        sm, eps = float(torch.tensor(spec.dice_smooth, dtype=f32)), float(torch.tensor(spec.dice_eps, dtype=f32))
        dw = float(torch.tensor(spec.dice, dtype=f32))
        u, dn = 2 * I + sm, P + T + sm
        present = T > 0
        clamped = dn < eps
        safe = torch.where(present & ~clamped, dn, torch.ones_like(dn))
        d = torch.where(present, 1 - u / torch.where(clamped, torch.full_like(dn, eps), safe), torch.zeros_like(dn))
        gno = torch.where(present & ~clamped, u / (safe * safe) / C, torch.zeros_like(dn))
        gyes = torch.where(present, torch.where(clamped, torch.full_like(dn, -2.0 / (eps * C)), gno - 2.0 / (safe * C)), torch.zeros_like(dn))
        dice = float((d.sum() / C).to(f32))
        gno32, gyes32 = (dw * gno).to(f32), (dw * gyes).to(f32)
        gsel = torch.where(onehot.bool(), gyes32[None, :].expand_as(p), gno32[None, :].expand_as(p))
        dot = torch.zeros_like(m)
        for c in range(C):
            dot = dot + p[:, c] * gsel[:, c]
        g = g + (p * (gsel - dot[:, None])) * kf[:, None]
    loss = float(torch.tensor((spec.ce * ce if spec.ce > 0 else 0.0) + (spec.dice * dice if spec.dice > 0 else 0.0), dtype=torch.float64).to(f32))
    return {"loss": loss, "ce": ce, "dice": dice, "dl": g.view(B, H, W, C).permute(0, 3, 1, 2).contiguous(), "preds": preds.view(B, H, W)}


# ------------------------------------------------------------------------------------------------ exact cases
EXACT_C, EXACT_SHAPE = 13, (2, 9, 13)


def exact_logits(winners, C):
    """(B, C, H, W) fp32 logits of +120 at each pixel's winner and -120 elsewhere: exp(-240) is 0 in fp32 and in fp64 it is 6e-105,
    so every softmax is one-hot in any arithmetic."""
    x = torch.full((winners.shape[0], C) + tuple(winners.shape[1:]), -120.0)
    x.scatter_(1, winners[:, None], 120.0)
    return x


def exact_winners(C=EXACT_C, shape=EXACT_SHAPE):
    g = torch.Generator().manual_seed(7)
    return torch.randint(0, C, shape, generator=g)
