"""Case table and references of the cross-entropy head's operator tests (test_gpu_ce_head_exact.py, test_ce_head_cases_cpu.py).

The head (csrc/ce_head.hip) is compared with torch's own fp64 cross entropy, label by label and column by column:

* logits come from two families, both exactly representable in bf16, so the fp32 NCHW tensor, the fp32 NHWC rows and the bf16 NHWC
  rows of a case hold the same values: ``ints`` (integers in [-3, 3]: most pixels tie, the first index must win) and ``far`` (even
  integers in [-120, 120]: exp(x - max) underflows for most classes and a pixel's loss term is near 100, so a kernel that dropped
  the max subtraction or formed -log(p[y]) fails);
* every label kind is built from one int64 map: about 15 % of the pixels carry a value outside [0, C) in the kind's own width,
  one class is absent, and the one-hot kind has a few all-zero pixels (class 0);
* three weight settings: none, random with w[2] = 0, and several zeros as a FLAIR config file has them.

NHWC_CASES run through flair_ce_head_nhwc (six instantiations: row stride 16 / 24 / 32 x fp32 / bf16), NCHW_CASES through
flair_ce_head, whose choice between the four-pixel and the one-pixel kernel routes_vec4 restates; every case names the kernel it
is written for.  This module needs no device."""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn.functional as F

import exact_cases as E

DTYPES = ("f32", "bf16")
KINDS = ("u8", "i32", "i64", "onehot")
CE_BLOCK_CAP = E.CE_BLOCK_CAP                   # ce_blocks(): at most 2 048 blocks of 256 threads
SMALL, MEDIUM, LARGE = (2, 9, 13), (3, 32, 24), E.CE_SHAPES[2]

# the project's bounds for this arithmetic (test_gpu_ops_exact.py holds the NCHW kernels to the same)
LOSS_RTOL = 2e-6          # |loss - ref| <= LOSS_RTOL * max(1, |ref|)
DL_ATOL, DL_RTOL = 1e-9, 1e-5   # max |dl - ref| <= DL_ATOL + DL_RTOL * max |ref|
MAXPROB_ATOL = 1e-6

IGNORED_U8 = (255, None)                                        # None: the case's C
IGNORED_I32 = (-1, None, 255, 2 ** 31 - 1)
IGNORED_I64 = IGNORED_I32 + (2 ** 32 + 3, -(2 ** 32) + 1, 2 ** 63 - 1)   # (int) of these: 3, 1, -1
IGNORE_SHARE = 0.15
ABSENT_CLASS = 1          # no pixel carries it (where C > 2)
ZERO_ONEHOT_PIXELS = 5    # all-zero one-hot pixels -> class 0


def loss_bound(ref):
    return LOSS_RTOL * max(1.0, abs(ref))


def dl_bound(ref_dl):
    return DL_ATOL + DL_RTOL * float(ref_dl.abs().max())


# ------------------------------------------------------------------------------------------------ routing, restated
def routes_vec4(HW, C, dl_ld, aligned):
    """ce_head(): the four-pixel kernel ce_main4_kernel<16 / 32> runs iff this holds, else ce_main_kernel.  dl_ld: row stride of
    dlogits_nhwc, 0 without one; aligned: logits and dlogits_nchw on 16 bytes and preds_u8 on 4."""
    return HW % 4 == 0 and (dl_ld == 0 or dl_ld <= (16 if C <= 16 else 32)) and aligned


def softmax_routes_vec4(HW, aligned):
    """softmax_argmax(): aligned = logits and maxprob on 16 bytes and preds_u8 on 4."""
    return HW % 4 == 0 and aligned


def nchw_kernel(C, shape, dl_ld, misalign):
    """The kernel flair_ce_head takes, and for the one-pixel kernel the reason."""
    HW = shape[1] * shape[2]
    if routes_vec4(HW, C, dl_ld, not misalign):
        return "main4_16" if C <= 16 else "main4_32"
    if HW % 4:
        return "scalar_odd_hw"
    return "scalar_misaligned" if misalign else "scalar_dl_ld"


def blocks(npix):
    return max(1, min((npix + 255) // 256, CE_BLOCK_CAP))


# ------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class NhwcCase:
    C: int
    ld: int
    shape: tuple
    family: str      # ints | far
    weight: str      # none | rand | zeros

    @property
    def name(self):
        return f"c{self.C}_ld{self.ld}_{'x'.join(map(str, self.shape))}_{self.family}_{self.weight}"

    @property
    def npix(self):
        return self.shape[0] * self.shape[1] * self.shape[2]

    def kernel(self, dt):
        return f"nhwc_{dt}_{self.ld}"

    @property
    def values(self):
        return self.C, self.shape, self.family, self.weight


@dataclass(frozen=True)
class NchwCase:
    C: int
    shape: tuple
    family: str
    weight: str
    dl_ld: int           # row stride of dlogits_nhwc (0: none)
    kernel: str          # what the case is written for (nchw_kernel)
    misalign: str = ""   # "" | logits | preds | dlogits: the pointer that sits one element off

    @property
    def name(self):
        return (f"c{self.C}_{'x'.join(map(str, self.shape))}_{self.family}_{self.weight}_dl{self.dl_ld}"
                + (f"_off_{self.misalign}" if self.misalign else ""))

    @property
    def npix(self):
        return self.shape[0] * self.shape[1] * self.shape[2]

    @property
    def values(self):
        return self.C, self.shape, self.family, self.weight


C_LD = [(1, 16), (13, 16), (16, 16), (13, 24), (17, 24), (19, 24), (13, 32), (19, 32), (32, 32)]


def _nhwc_cases():
    out = []
    fam = ("ints", "far")
    wts = ("rand", "none")
    for k, (C, ld) in enumerate(C_LD):
        # both shapes for every (C, ld); the family and the weight setting alternate so that every row stride meets both of each
        out.append(NhwcCase(C, ld, SMALL, fam[k % 2], wts[(k // 2) % 2]))
        out.append(NhwcCase(C, ld, MEDIUM, fam[(k + 1) % 2], wts[(k // 2 + 1) % 2]))
    out.append(NhwcCase(19, 32, MEDIUM, "ints", "zeros"))       # the YAML-like weights: classes 12.. weigh nothing
    out.append(NhwcCase(13, 16, LARGE, "far", "rand"))          # past the grid cap: the only large cases
    out.append(NhwcCase(19, 32, LARGE, "ints", "rand"))
    return out


NHWC_CASES = _nhwc_cases()

NCHW_CASES = [
    # four-pixel kernel, both instantiations, with and without NHWC rows at their limit
    NchwCase(13, MEDIUM, "ints", "rand", 16, "main4_16"),
    NchwCase(16, MEDIUM, "far", "none", 0, "main4_16"),
    NchwCase(19, MEDIUM, "far", "rand", 24, "main4_32"),
    NchwCase(19, MEDIUM, "ints", "zeros", 32, "main4_32"),
    NchwCase(32, MEDIUM, "ints", "rand", 32, "main4_32"),
    # one-pixel kernel: H*W % 4 != 0
    NchwCase(13, SMALL, "far", "rand", 16, "scalar_odd_hw"),
    NchwCase(17, SMALL, "ints", "rand", 24, "scalar_odd_hw"),
    NchwCase(32, SMALL, "far", "none", 32, "scalar_odd_hw"),
    NchwCase(1, SMALL, "ints", "rand", 0, "scalar_odd_hw"),
    # one-pixel kernel: NHWC rows wider than the four-pixel kernel's register row
    NchwCase(13, MEDIUM, "ints", "rand", 24, "scalar_dl_ld"),
    NchwCase(13, MEDIUM, "far", "none", 32, "scalar_dl_ld"),
    # one-pixel kernel: a pointer off its alignment (the values of the first two cases: the results must be theirs)
    NchwCase(13, MEDIUM, "ints", "rand", 16, "scalar_misaligned", misalign="logits"),
    NchwCase(13, MEDIUM, "ints", "rand", 16, "scalar_misaligned", misalign="preds"),
    NchwCase(16, MEDIUM, "far", "none", 0, "scalar_misaligned", misalign="dlogits"),
]


# ------------------------------------------------------------------------------------------------ inputs
def _seed(*parts):
    return sum((i + 1) * ord(ch) for i, ch in enumerate("|".join(map(str, parts)))) % (2 ** 31)


def logits_of(C, shape, family):
    """fp32 (B, C, H, W), every value a bf16 number."""
    B, H, W = shape
    g = torch.Generator().manual_seed(_seed("x", C, shape, family))
    if family == "ints":
        x = E.ints((B, C, H, W), g, -3, 3)
    else:
        assert family == "far"
        x = E.ints((B, C, H, W), g, -60, 60) * 2
    assert torch.equal(x.bfloat16().float(), x)
    return x


def weight_of(C, setting):
    if setting == "none":
        return None
    if setting == "zeros":      # as in a FLAIR config: the last classes weigh nothing
        w = torch.ones(C)
        w[12:] = 0
        assert C > 12 and int((w == 0).sum()) >= 2
        return w
    assert setting == "rand"
    w = torch.rand(C, generator=torch.Generator().manual_seed(_seed("w", C))) + 0.1
    if C > 2:
        w[2] = 0.0
    return w


def _cycle(values, C, n):
    vals = [C if v is None else v for v in values]
    return torch.tensor([vals[i % len(vals)] for i in range(n)], dtype=torch.int64)


def labels_of(C, shape):
    """dict: y (int64, the valid map; ABSENT_CLASS absent where C > 2), ign (bool), u8 / i32 / i64 (the integer kinds, the ignored
    pixels carrying the kind's out-of-range values in turn), onehot (fp32 one-hot of y with ZERO_ONEHOT_PIXELS all-zero pixels)
    and y_onehot (what the one-hot means: those pixels are class 0, nothing is ignored)."""
    B, H, W = shape
    g = torch.Generator().manual_seed(_seed("y", C, shape))
    y = torch.randint(0, C, (B, H, W), generator=g)
    if C > 2:
        y[y == ABSENT_CLASS] = C - 1
    ign = torch.rand((B, H, W), generator=g) < IGNORE_SHARE
    n = int(ign.sum())
    out = {"y": y, "ign": ign}
    for kind, vals, dtype in (("u8", IGNORED_U8, torch.uint8), ("i32", IGNORED_I32, torch.int32), ("i64", IGNORED_I64, torch.int64)):
        lab = y.clone()
        lab[ign] = _cycle(vals, C, n)
        assert n >= len(vals), "every ignored value appears"
        out[kind] = lab.to(dtype)
        assert torch.equal(out[kind].to(torch.int64), lab), "the kind holds its values"
    onehot = F.one_hot(y, C).permute(0, 3, 1, 2).float().contiguous()
    zero = torch.zeros(B * H * W, dtype=torch.bool)
    zero[torch.nonzero(y.flatten() != 0).flatten()[:ZERO_ONEHOT_PIXELS]] = True
    zero = zero.view(B, H, W)
    onehot.permute(0, 2, 3, 1)[zero] = 0
    out["onehot"] = onehot
    out["y_onehot"] = torch.where(zero, torch.zeros_like(y), y)
    out["zero"] = zero
    return out


def expected_targets(lab, C):
    """What targets_i32 holds for an integer label map: (exact, mask) - the label itself where int32 holds it; elsewhere (mask
    False) any value outside [0, C)."""
    l64 = lab.to(torch.int64)
    fits = (l64 >= -(2 ** 31)) & (l64 < 2 ** 31)
    return l64, fits


# ------------------------------------------------------------------------------------------------ reference
def reference_of(x, y, valid, w):
    """torch's fp64 cross entropy with autograd, the fp64 softmax argmax and the confusion matrix over the valid pixels.
    x (B, C, H, W) fp32; y int64 (B, H, W); valid bool (B, H, W); w fp32 (C,) or None."""
    from oracle import seg_step
    C = x.shape[1]
    xd = x.double().requires_grad_(True)
    tgt = torch.where(valid, y, torch.full_like(y, -100))
    loss = F.cross_entropy(xd, tgt, weight=None if w is None else w.double(), ignore_index=-100)
    (dl,) = torch.autograd.grad(loss, xd)
    with torch.no_grad():
        prob = torch.softmax(x.double(), 1)
        preds = prob.argmax(1)
        maxprob = prob.max(1).values
    cm = seg_step.confusion_matrix_np(y[valid].numpy(), preds[valid].numpy(), C)
    return {"loss": float(loss.detach()), "dl": dl, "preds": preds, "maxprob": maxprob, "confmat": cm}


@functools.lru_cache(maxsize=4)
def case_values(C, shape, family, weight):
    """Inputs of a case and its two references: "int" for the integer label kinds (15 % ignored), "onehot" for the one-hot."""
    x, w, lab = logits_of(C, shape, family), weight_of(C, weight), labels_of(C, shape)
    ref_int = reference_of(x, lab["y"], ~lab["ign"], w)
    ref_oh = reference_of(x, lab["y_onehot"], torch.ones_like(lab["ign"]), w)
    return {"x": x, "w": w, "lab": lab, "int": ref_int, "onehot": ref_oh}


def nhwc_rows(x, ld, fill=0.0):
    """(B, C, H, W) fp32 -> (B*H*W, ld) fp32 rows, the padded columns holding `fill`."""
    B, C, H, W = x.shape
    rows = torch.full((B * H * W, ld), fill, dtype=torch.float32)
    rows[:, :C] = x.permute(0, 2, 3, 1).reshape(-1, C)
    return rows


# ------------------------------------------------------------------------------------------------ the kernel's arithmetic in fp32
def kernel_arithmetic_f32(x, y, valid, w):
    """The kernels' arithmetic restated in fp32 on the CPU: max, exp(x - m), the sum in class order, log(sum) - (x_y - m), and
    (p - onehot) * w / den with p = e * (1 / sum).  Block sums of 256 pixels in fp32, their sum in fp64 (ce_sum_kernel).
    Returns loss (float), dl (B, C, H, W) fp32, preds."""
    B, C, H, W = x.shape
    f32 = torch.float32
    rows = x.permute(0, 2, 3, 1).reshape(-1, C).to(f32)
    yy = torch.where(valid, y, torch.zeros_like(y)).reshape(-1)
    ok = valid.reshape(-1)
    m = rows.max(1).values
    e = torch.exp(rows - m[:, None])
    s = torch.zeros_like(m)
    for c in range(C):
        s = s + e[:, c]
    p = e * (1.0 / s)[:, None]
    preds = p.argmax(1)      # (first index among equals, as the kernel's strict > keeps it)
    wy = (torch.ones(C) if w is None else w).to(f32)[yy] * ok.to(f32)
    xy = rows.gather(1, yy[:, None])[:, 0]
    term = wy * (torch.log(s) - (xy - m))
    npix = rows.shape[0]
    pad = (-npix) % 256
    part = lambda v: torch.cat([v, torch.zeros(pad)]).view(-1, 256).sum(1, dtype=f32)
    den = part(wy).double().sum().to(f32)
    loss = (part(term * ok.to(f32)).double().sum() / den.double()).to(f32)
    onehot = torch.zeros_like(rows)
    onehot[torch.arange(npix), yy] = ok.to(f32)
    dl = (p - onehot) * (wy * (1.0 / den))[:, None]
    return float(loss), dl.view(B, H, W, C).permute(0, 3, 1, 2).contiguous(), preds.view(B, H, W)


# ------------------------------------------------------------------------------------------------ confusion matrices for flair_jaccard
def jaccard_matrices():
    """name -> int64 confusion matrix: C = 1 and C = 32, absent classes (zero row and column), all zeros, counts near 2^40."""
    g = torch.Generator().manual_seed(40)
    big = torch.randint(2 ** 40 - 1000, 2 ** 40 + 1000, (13, 13), generator=g)
    absent = torch.randint(0, 50, (13, 13), generator=g)
    absent[3, :] = 0
    absent[:, 3] = 0
    absent[7, :] = 0      # class 7: never a target, sometimes predicted
    c32 = torch.randint(0, 1000, (32, 32), generator=g)
    c32[31, :] = 0
    c32[:, 31] = 0
    return {"c1": torch.tensor([[17]]), "c1_empty": torch.tensor([[0]]), "c32": c32, "absent": absent,
            "zeros": torch.zeros(19, 19, dtype=torch.int64), "near_2pow40": big,
            "prefilled_2pow40": torch.full((19, 19), 2 ** 40) + torch.randint(0, 500, (19, 19), generator=g)}
