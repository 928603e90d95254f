"""Operator cases of flair_add_rowvec_nhwc, x[n][h][w][c] += v[n][h] on an NHWC tensor, and their expected bits (torch, CPU).

One shape, N=3, H=5, W=2, C=24: the three extents differ and C is no power of two, so a swapped n / h / w index or a wrong channel
stride lands on another value of v.  fp32 expectation: x + v[:, :, None, None].  bf16 expectation: (x.float() + v).to(bfloat16) —
the sum in fp32, rounded once, to nearest even.  Four planted elements sit on or next to a bf16 rounding tie:

    x          v                result
    1.0        2^-8             1.0         (tie, the even neighbour is below)
    1 + 2^-7   2^-8             1 + 2^-6    (tie, the even neighbour is above)
    3.0        2^-7 + 2^-20     3.015625    (just above the tie: up, whatever the parity)
    -1.0       -2^-8            -1.0        (tie on the negative side)

v is per (n, h), so each planted element has a row of its own; every element of that row sees the planted v.
"""
import torch

N, H, W, C = 3, 5, 2, 24

# (n, h, w, c) of the planted element, x, v[n][h], expected bf16 result
TIES = [
    ((0, 0, 0, 0), 1.0, 2.0 ** -8, 1.0),
    ((0, 3, 1, 23), 1.0 + 2.0 ** -7, 2.0 ** -8, 1.0 + 2.0 ** -6),
    ((1, 2, 1, 8), 3.0, 2.0 ** -7 + 2.0 ** -20, 3.015625),
    ((2, 4, 0, 17), -1.0, -(2.0 ** -8), -1.0),
]


def case(dtype):
    """(x NHWC in `dtype`, v fp32 (N, H), expected NHWC in `dtype`) for dtype torch.float32 / torch.bfloat16; CPU tensors."""
    g = torch.Generator().manual_seed(45)
    x = torch.randn(N, H, W, C, generator=g).to(dtype)
    v = torch.randn(N, H, generator=g)
    for (n, h, w, c), xv, vv, _ in TIES:
        x[n, h, w, c] = xv
        v[n, h] = vv
    if dtype == torch.float32:
        want = x + v[:, :, None, None]
    else:
        want = (x.float() + v[:, :, None, None]).to(torch.bfloat16)
    return x, v, want


def wide_case():
    """fp32, C = 512, (2, 16, 16) rows: the bottleneck of two 512 x 512 tiles.  (x NHWC, v); the expectation is
    flair_add_rowvec_nchw on the transposed tensor."""
    g = torch.Generator().manual_seed(46)
    return torch.randn(2, 16, 16, 512, generator=g), torch.randn(2, 16, generator=g)
