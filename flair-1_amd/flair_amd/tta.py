"""Test-time augmentation over the D4 group the network is trained under (tasks_utils.py:37-41 of the reference: V-flip, H-flip,
rot90), DESIGN §10.

A transform code is ``data_feed.pack_d4``'s: bit 0 V-flip, bit 1 H-flip, bits 2-3 the rot90 count k, meaning
``rot90^k(hflip(vflip(a)))`` with numpy's counter-clockwise rot90.  For codes t1..tn

    S     = sum_k T_k^-1(softmax(f(T_k(x))))     fp32, in list order
    preds = the lowest-index class of the largest S
    prob  = max S / n                             one fp32 division

``f`` is the model's eval-mode logits.  On the device it is one permutation kernel in front of each forward (``ops.d4_transform``) and
one accumulate kernel behind it (``ops.tta_accumulate``); the last accumulate writes class and probability, no probability tensor is
ever written.
"""
from __future__ import annotations

import torch

from . import ops

FLIPS = [0, 1, 2, 3]
D4 = [0, 1, 4, 5, 8, 9, 12, 13]   # the eight distinct group elements (an H-flip is a V-flip behind rot90^2)
MAX_PASSES = 16


def tta_codes(spec):
    """The list of transform codes a ``tta`` argument stands for, or None when it switches the ensemble off.
    None, "none", []: off; "flips": [0, 1, 2, 3]; "d4": the eight group elements; a list of 1 to 16 ints in 0..15: itself."""
    if spec is None:
        return None
    if isinstance(spec, str):
        if spec == "none":
            return None
        if spec == "flips":
            return list(FLIPS)
        if spec == "d4":
            return list(D4)
        raise ValueError(f"tta {spec!r}: one of None, 'none', 'flips', 'd4' or a list of 1 to {MAX_PASSES} transform codes in 0..15")
    if not isinstance(spec, (list, tuple)):
        raise ValueError(f"tta {spec!r}: one of None, 'none', 'flips', 'd4' or a list of 1 to {MAX_PASSES} transform codes in 0..15")
    if len(spec) == 0:
        return None
    if len(spec) > MAX_PASSES:
        raise ValueError(f"tta lists at most {MAX_PASSES} transform codes, not {len(spec)}")
    codes = []
    for c in spec:
        if isinstance(c, bool) or not isinstance(c, int) or not 0 <= c <= 15:
            raise ValueError(f"tta transform code {c!r}: an int in 0..15 (bit 0 V-flip, bit 1 H-flip, bits 2-3 rot90 count)")
        codes.append(int(c))
    return codes


def check_codes(codes, H, W):
    """An odd rot90 count turns an H x W tile into a W x H one, which no model here takes in the same batch"""
    if H != W and any(c & 4 for c in codes):
        raise ValueError(f"tta codes {[c for c in codes if c & 4]} have an odd rot90 count: they need square tiles, not {H} x {W}")


@torch.no_grad()
def tta_predict(logits_fn, x, codes, want_prob=False, quarter=False):
    """The ensemble of ``logits_fn`` over ``codes`` for the fp32 (B, C, H, W) batch ``x``: uint8 (B, h, w) classes and, with
    ``want_prob``, their fp32 mean probability.  ``logits_fn(T(x))`` returns fp32 (B, classes, h, w) logits, h x w the tile's extent
    or, with ``quarter``, a quarter of it: those are resized x4 per pixel inside the accumulate kernel and the result is tile-sized.
    Each pass's logits are consumed on the current stream before the next forward runs, so ``logits_fn`` may hand out the same
    tensor every time."""
    codes = tta_codes(list(codes))
    if codes is None:
        raise ValueError("tta_predict needs at least one transform code")
    if x.dim() != 4:
        raise ValueError("tta_predict takes a (B, C, H, W) batch")
    H, W = x.shape[-2:]
    check_codes(codes, H, W)
    x = x.detach().float().contiguous()
    n = len(codes)
    acc = preds = prob = None
    for k, code in enumerate(codes):
        logits = logits_fn(x if code == 0 else ops.d4_transform(x, code)).detach().float().contiguous()
        B, C, h, w = logits.shape
        up = 4 if quarter else 1
        if k == 0:
            check_codes(codes, h, w)
            if n > 1:
                acc = torch.empty(B, C, h * up, w * up, dtype=torch.float32, device=logits.device)
        if k == n - 1:
            preds = torch.empty(B, h * up, w * up, dtype=torch.uint8, device=logits.device)
            prob = torch.empty(B, h * up, w * up, dtype=torch.float32, device=logits.device) if want_prob else None
        ops.tta_accumulate(logits, code, acc=acc, first=k == 0, preds=preds, prob=prob, n=n, quarter=quarter)
    return (preds, prob) if want_prob else preds
