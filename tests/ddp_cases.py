"""Two data-parallel replicas of the oracle U-Net on the CPU (no device needed): what one SegTrainer step with the gradient
exchange has to compute, stated with the oracle's own modules.

  * both replicas start from rank 0's weights (DDP's initial broadcast), rank r is fed its own batch;
  * BatchNorm batch statistics stay PER RANK (no SyncBN, like the reference's 'ddp' strategy);
  * the gradient every rank applies is the MEAN over the ranks;
  * every rank ends the step holding RANK 0's running statistics (torch DDP broadcast_buffers=True).

`two_replica_step` returns that step in a given dtype; `wrong_variants` the three plausible mistakes (global BatchNorm
statistics, rank 0's gradient alone, sum instead of mean).  tests/test_ddp_cases_cpu.py asserts that the mistakes lie far outside
the fp32 noise of the right answer, tests/test_gpu_ddp.py runs the HIP trainer against it."""
import copy

import torch
import torch.nn as nn

IN_CH, CLASSES, SEED0 = 5, 13, 100     # rank r's OWN initial weights are seeded_model(5, 13, SEED0 + r): only rank 0's may survive
HW = (96, 128)                         # non-square, 3 x 4 bottleneck pixels
WORLD = 2
LR = 0.05


def batch(rank, hw=HW, n=2):
    """Rank r's batch: per-rank seed, randn then randint."""
    g = torch.Generator().manual_seed(2022 + rank)
    return torch.randn(n, IN_CH, *hw, generator=g), torch.randint(0, CLASSES, (n, *hw), generator=g, dtype=torch.uint8)


def initial_model(rank=0):
    from oracle import unet_resnet34 as om
    return om.seeded_model(IN_CH, CLASSES, SEED0 + rank)


def _fwd_bwd(model, x, lab, dtype):
    m = copy.deepcopy(model).to(dtype).train()
    loss = nn.functional.cross_entropy(m(x.to(dtype)), lab.long())
    loss.backward()
    return m, float(loss.detach())


def _grads(m):
    return {k: p.grad.detach().double() for k, p in m.named_parameters()}


def _buffers(m):
    return {k: b.detach().double() for k, b in m.named_buffers()}


def two_replica_step(dtype=torch.float64, hw=HW):
    """One data-parallel step of WORLD replicas from rank 0's initial weights.  Returns a dict: 'loss' [per rank],
    'rank_grads' [per rank {name: fp64 tensor}], 'mean_grad' {name: tensor}, 'buffers' [per rank {name: tensor}] (each
    replica's OWN running statistics after the step; every rank must end up with buffers[0])."""
    start = initial_model(0)
    reps = [_fwd_bwd(start, *batch(r, hw), dtype) for r in range(WORLD)]
    rank_grads = [_grads(m) for m, _ in reps]
    # the exchange in the arithmetic of the dtype under test (one addition per element, then the division), held as fp64
    mean = {k: ((rank_grads[0][k].to(dtype) + rank_grads[1][k].to(dtype)) / WORLD).double() for k in rank_grads[0]}
    return {"loss": [l for _, l in reps], "rank_grads": rank_grads, "mean_grad": mean, "buffers": [_buffers(m) for m, _ in reps]}


def wrong_variants(step64, hw=HW):
    """Three gradients a wrong exchange would apply, in fp64: {name: {param: tensor}}."""
    start = initial_model(0)
    xs, labs = zip(*[batch(r, hw) for r in range(WORLD)])
    glob, _ = _fwd_bwd(start, torch.cat(xs), torch.cat(labs), torch.float64)   # one model, the global batch: SyncBN-like statistics
    return {"global_bn": _grads(glob),
            "rank0_only": step64["rank_grads"][0],
            "sum": {k: step64["rank_grads"][0][k] + step64["rank_grads"][1][k] for k in step64["mean_grad"]}}


def tensor_errs(got, truth):
    """Per-tensor relative max-norm distance, as test_gpu_model's gradient comparisons measure it."""
    return {k: float((got[k].double() - truth[k]).abs().max() / (truth[k].abs().max() + 1e-12)) for k in truth}


def quantiles(errs):
    s = sorted(errs.values())
    return s[len(s) // 2], s[min(len(s) - 1, int(0.9 * len(s)))], s[-1]


def running_stat_gap(buffers):
    """How far rank 1's running statistics lie from rank 0's, per tensor, relative to the size of rank 0's own update
    (running_mean starts at 0, running_var at 1 and keeps 0.9 of that after one step at momentum 0.1)."""
    out = {}
    for k, b0 in buffers[0].items():
        if k.endswith("running_mean"):
            scale = b0.abs().max()
        elif k.endswith("running_var"):
            scale = (b0 - 0.9).abs().max()
        else:
            continue
        out[k] = float((buffers[1][k] - b0).abs().max() / (scale + 1e-12))
    return out
