"""Host-side pieces of the fused trainer's validation: the cross-rank reduction of its accumulators (gloo, host tensors)."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_state(rank):
    """(batch losses, confusion matrix) a rank has accumulated: different on every rank, a different number of batches too."""
    g = torch.Generator().manual_seed(100 + rank)
    losses = torch.rand(3 + rank, generator=g, dtype=torch.float64) + 0.5
    cm = torch.randint(0, 1000, (4, 4), generator=g, dtype=torch.int64)
    return losses, cm


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from flair_amd import reduce_validation_state
    losses, cm = _rank_state(rank)
    loss_sum, count = losses.sum(), torch.tensor(float(len(losses)), dtype=torch.float64)
    reduce_validation_state(loss_sum, count, cm, None)
    out[rank] = (loss_sum.item(), count.item(), cm.tolist())
    dist.destroy_process_group()


def test_reduce_validation_state_world2_gloo():
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    states = [_rank_state(r) for r in range(2)]
    all_losses = torch.cat([s[0] for s in states])
    cm_sum = (states[0][1] + states[1][1]).tolist()
    for r in range(2):
        loss_sum, count, cm = out[r]
        assert count == len(all_losses) == 7 and cm == cm_sum
        assert abs(loss_sum - all_losses.sum().item()) <= 1e-12
        # MeanMetric over the concatenated batches of one process
        assert abs(loss_sum / count - all_losses.mean().item()) <= 1e-12
