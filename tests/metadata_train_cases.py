"""Device-free cases of the training form of the bottleneck row add: flair_add_rowvec_nhwc_to (y = T(float(x) + v[n][h]), out of
place) and its gradient flair_rowvec_grad_nhwc (dv[n][h] = sum over w, c of dx[n][h][w][c]), with their expectations (torch, CPU).

Exact cases: integer values in [-8, 8] are bf16 numbers, and a row of the largest shape sums 16 * 512 of them, below 2**17 in
magnitude: every partial sum in any order is an integer below 2**24 and therefore exact in fp32.  The kernel's result must equal
the int64 sum bit for bit, whatever its order.

Random cases: for fp32 accumulation of n terms in ANY order, |computed - exact| <= (n - 1) * u * sum |x_i| with u = 2**-24 (Higham,
Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4, first order in u; the inputs are bf16 or fp32 numbers and enter
the sum exactly)."""
import torch

ADD_SHAPES = [(1, 1, 1, 8), (2, 3, 5, 32), (2, 16, 16, 512)]
GRAD_SHAPES = [
    (1, 1, 1, 8),       # one 16-byte chunk (bf16), two (fp32): one lane works
    (1, 2, 7, 24),      # a row of 21 (bf16) / 42 (fp32) chunks: not a multiple of the workgroup's stride of 256
    (3, 2, 3, 512),     # odd N; 192 / 384 chunks per row: the second pass over the row is partial in fp32
    (2, 16, 16, 512),   # the bottleneck: 1024 / 2048 chunks per row, every lane loops
]
U = 2.0 ** -24

# flair_unet_workspace_bytes(B=2, H=160, W=128) of the 5-band 13-class executor, (training, eval) per compute dtype, as reported before
# the training request existed: the request adds one bottleneck tensor to a training forward and must fit inside the same bound
WORKSPACE_2x160x128 = {"f32": (473325312, 236561408), "bf16": (312342272, 118905856)}


def _gen(shape):
    return torch.Generator().manual_seed(1000 + sum(s * (i + 1) for i, s in enumerate(shape)))


def int_case(shape, dtype):
    """dx with integer values in [-8, 8] and the exact row sums as fp32."""
    dx = torch.randint(-8, 9, shape, generator=_gen(shape)).to(dtype)
    want = dx.to(torch.int64).sum(dim=(2, 3))
    assert int(want.abs().max()) < 2 ** 17
    return dx, want.to(torch.float32)


def normal_case(shape, dtype):
    """dx ~ N(0, 1) rounded to dtype, the fp64 row sums and the any-order bound per row."""
    dx = torch.randn(shape, generator=_gen(shape)).to(dtype)
    d64 = dx.to(torch.float64)
    n = shape[2] * shape[3]
    return dx, d64.sum(dim=(2, 3)), (n - 1) * U * d64.abs().sum(dim=(2, 3))


def add_case(shape, dtype):
    """x, v and T(float(x) + v[n][h]) — the arithmetic of add_rowvec_nhwc_kernel: one fp32 add, one rounding to T."""
    g = _gen(shape)
    x = torch.randn(shape, generator=g).to(dtype)
    v = torch.randn(shape[0], shape[1], generator=g)
    want = (x.to(torch.float32) + v[:, :, None, None]).to(dtype)
    return x, v, want


def rel_max_err(got, truth):
    """Relative max-norm error of one tensor, as parity_helpers.grad_errs measures every gradient tensor."""
    return float((got.detach().cpu().double() - truth.double()).abs().max() / (truth.double().abs().max() + 1e-12))
