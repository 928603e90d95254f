"""Two data-parallel ranks sharing the one GPU of a test box (gloo carries the HIP tensors; the 8-GPU RCCL run
is the driver's): the native backward's per-stage events, the side-stream bucketed all-reduce and the folded 1/world SGD
step must give every rank the same weights, equal to a single-process step on the mean of the two ranks' gradients
computed with PER-RANK BatchNorm statistics (no SyncBN, like the reference's DDP — SURVEY.md §8e).

Below the two original tests: ONE pair of workers (`suite`) runs every further configuration in sequence inside one gloo group —
the first step against the two-replica CPU oracle of tests/ddp_cases.py, bucket sizes x overlap, one-rank sub-groups with
force_exchange, validation with world = 2 — and the tests assert on what the workers sent back."""
import hashlib
import os
import socket
import time
from multiprocessing.connection import wait as _wait_any

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _batch(rank):
    g = torch.Generator().manual_seed(2022 + rank)  # per-rank seed, SURVEY.md §8d config 3
    return torch.randn(2, 5, 64, 64, generator=g), torch.randint(0, 13, (2, 64, 64), generator=g, dtype=torch.uint8)


def _model(seed):
    import flair_amd
    torch.manual_seed(seed)
    return flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=13, compute_dtype="f32")


def _worker(rank, world, port, overlap, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import flair_amd
    dev = torch.device("cuda:0")
    model = _model(100 + rank).to(dev).train()  # different initial weights: the trainer must broadcast rank 0's
    trainer = flair_amd.SegTrainer(model, lr=0.05, overlap=overlap)
    img, lab = _batch(rank)
    for _ in range(2):
        loss = trainer.train_step(img.to(dev), lab.to(dev))
    torch.cuda.synchronize()
    # eval-mode forward on each rank WITHOUT any collective of its own: the running statistics must already be rank 0's
    model.eval()
    with torch.no_grad():
        ev = model(_batch(7)[0].to(dev)).cpu()
    out[rank] = (model.flat_parameters().detach().cpu(), float(loss), model.flat_buffers().detach().cpu(), ev)
    dist.destroy_process_group()


@pytest.mark.parametrize("overlap", [True, False])
def test_two_ranks_one_gpu_match_single_process_average(dev, overlap):
    import flair_amd
    ctx = mp.get_context("spawn")
    out = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, overlap, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(300)
        assert p.exitcode == 0
    w0, w1 = out[0][0], out[1][0]
    assert torch.equal(w0, w1)  # replicas stay bit-identical
    # single-process replay: two replicas from rank 0's initial weights, gradients averaged by hand
    reps = [_model(100).to(dev).train() for _ in range(2)]
    trainers = [flair_amd.SegTrainer(m, lr=0.05) for m in reps]
    for _ in range(2):
        for r, (m, t) in enumerate(zip(reps, trainers)):
            img, lab = _batch(r)
            t.lr = 0.0  # gradients only
            t.train_step(img.to(dev), lab.to(dev))
        mean = (trainers[0].grads + trainers[1].grads) / 2
        for m in reps:
            m.flat_parameters().data.add_(mean, alpha=-0.05)
    ref = reps[0].flat_parameters().detach().cpu()
    assert torch.equal(reps[0].flat_parameters(), reps[1].flat_parameters())
    err = (w0 - ref).abs().max().item()
    assert err < 2e-6, err  # (g0 + g1) * (lr / 2) vs ((g0 + g1) / 2) * lr: rounding only
    start = _model(100).to(dev).flat_parameters().detach().cpu()
    assert (w0 - start).abs().max() > 1e-4  # and the step did move the weights
    # torch DDP broadcast_buffers=True (tasks.py:83-88 keeps the default): every rank holds RANK 0's running statistics — the
    # ones a single process fed rank 0's batches accumulates — so rank 1's eval logits equal rank 0's bit for bit
    assert torch.equal(out[0][2], out[1][2])
    assert torch.equal(out[0][3], out[1][3])
    b_ref = reps[0].flat_buffers().detach().cpu()
    assert torch.allclose(out[1][2], b_ref, rtol=1e-5, atol=1e-6), float((out[1][2] - b_ref).abs().max())
    assert not torch.allclose(out[1][2], reps[1].flat_buffers().detach().cpu(), rtol=1e-3, atol=1e-4)   # (rank 1's own differ)


def test_bench_n_gt_1_branch_runs_end_to_end_on_gloo():
    """Every line of bench.py's N>1 branch (self-spawned ranks, process group, per-rank tiles, barrier + max-over-ranks timing,
    the exchange object) executed once before the driver's 8-GPU RCCL run: two ranks on the one GPU of this box, gloo instead
    of RCCL (FLAIR_BENCH_BACKEND / FLAIR_BENCH_DEVICES), small tiles."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, FLAIR_BENCH_BACKEND="gloo", FLAIR_BENCH_DEVICES="0,0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--batch", "2",
                        "--size", "64", "--dtype", "f32", "--no-cpu-baseline", "--full"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["config"]["global_batch"] == 4 and line["scaling"] == "weak"
    ex = line["exchange"]
    assert ex["collective_ranks"] == 2 and ex["backend"] == "gloo" and len(ex["per_rank_ms_per_step"]) == 2
    assert line["value"] > 0 and abs(line["value"] - 4 * 3 / (line["ms_per_step"] * 3e-3)) < 1e-2 * line["value"]
    assert "surface" not in line and "cpu_baseline" not in line   # rank 0 at N = 1 only


# ====================================================================================== one pair of workers, every configuration
SUITE_TIME_LIMIT = 300          # seconds for the whole pair; a worker alive after it is killed and the test fails
FIRST_STEP_BOUNDS = (2.0, 2.0, 3.0)     # measured 1.36 / 1.31 / 1.12: test_first_step_matches_the_two_replica_oracle
BUCKET_SIZES = (0, 1 << 18, 1 << 30)   # every stage its own bucket / the default / everything in one
VAL_WEIGHT_ZERO = 4


def _digest(*tensors):
    """Bit-identity across processes without shipping 98 MB per tensor: SHA-256 of the raw bytes."""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _val_batch(rank, j):
    g = torch.Generator().manual_seed(4000 + 10 * rank + j)
    return torch.randn(2, 5, 64, 64, generator=g), torch.randint(0, 13, (2, 64, 64), generator=g, dtype=torch.uint8)


def _val_weight():
    w = torch.linspace(0.5, 1.5, 13)
    w[VAL_WEIGHT_ZERO] = 0.0
    return w


def _hip_model(state_dict, dev):
    import flair_amd
    m = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=13, compute_dtype="f32")
    m.load_state_dict(state_dict, strict=True)
    return m.to(dev).train()


def _suite_worker(rank, port, out_dir):
    t0 = time.monotonic()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    import flair_amd
    import ddp_cases as D
    dev = torch.device("cuda:0")
    own = D.initial_model(rank).state_dict()      # rank 1 starts from OTHER weights: the trainer's broadcast must replace them
    img, lab = (t.to(dev) for t in D.batch(rank))
    res = {"seconds": {}}

    # ---- (A) the first step, for the oracle
    m = _hip_model(own, dev)
    tr = flair_amd.SegTrainer(m, lr=D.LR)
    loss = tr.train_step(img, lab)
    torch.cuda.synchronize()
    names = [n for n, _ in m.named_parameters()]
    res["first"] = {"loss": float(loss),
                    "mean_grad": dict(zip(names, [(v / 2).cpu() for v in m._grad_views(tr.grads)])),
                    "buffers": {k: b.detach().cpu().clone() for k, b in m.named_buffers()},
                    "flat_buffers": m.flat_buffers().detach().cpu().clone()}
    del m, tr
    res["seconds"]["first"] = time.monotonic() - t0

    # ---- (B) bucket boundaries and overlap are invisible: two steps under each of the six settings.  The first setting's
    # state stays on the device and the others are compared with it there; its digest goes home for the comparison across ranks
    res["buckets"] = {}
    first = None
    for mbe in BUCKET_SIZES:
        for overlap in (True, False):
            m = _hip_model(own, dev)
            tr = flair_amd.SegTrainer(m, lr=D.LR, overlap=overlap, min_bucket_elems=mbe)
            start = m.flat_parameters().detach().clone()
            for _ in range(2):
                loss = tr.train_step(img, lab)
            torch.cuda.synchronize()
            state = {"weights": m.flat_parameters().detach().clone(), "grads": tr.grads.clone(), "buffers": m.flat_buffers().detach().clone()}
            if first is None:
                first = state
                res["buckets_first_digest"] = {k: _digest(v) for k, v in first.items()}
            res["buckets"][(mbe, overlap)] = {
                "same_as_first": {k: bool(torch.equal(v.view(torch.int32), first[k].view(torch.int32))) for k, v in state.items()},
                "loss": float(loss), "moved": float((m.flat_parameters() - start).abs().max()),
                "finite": bool(torch.isfinite(m.flat_parameters()).all() and torch.isfinite(tr.grads).all()),
                "bucket_ranges": list(tr.buckets), "bucket_stage": list(tr._bucket_stage), "stage_ranges": m.stage_ranges()}
            del m, tr, start, state
    del first
    res["seconds"]["buckets"] = time.monotonic() - t0

    # ---- (C) group= and force_exchange: a one-rank group of this rank's own; both ranks create both groups (a collective)
    groups = [dist.new_group([0]), dist.new_group([1])]
    res["group"] = {}
    for overlap in (True, False):
        got = {}
        for kind in ("exchange", "plain"):
            m = _hip_model(own, dev)
            tr = flair_amd.SegTrainer(m, lr=D.LR, group=groups[rank], overlap=overlap, force_exchange=(kind == "exchange"))
            for _ in range(2):
                loss = tr.train_step(img, lab)
            torch.cuda.synchronize()
            got[kind] = {"state": [m.flat_parameters().detach().clone(), tr.grads.clone(), m.flat_buffers().detach().clone()],
                         "loss": float(loss), "world": tr.world, "exchange": bool(tr.exchange), "src0": tr._src0,
                         "stem_weights": _digest(m.flat_parameters()[:4096])}
            del m, tr
        got["same_state"] = all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                                for a, b in zip(got["exchange"].pop("state"), got["plain"].pop("state")))
        res["group"][overlap] = got
    res["seconds"]["group"] = time.monotonic() - t0

    # ---- (D) validation with world = 2: two batches of this rank's own, class weights with a zero
    m = _hip_model(own, dev)
    tr = flair_amd.SegTrainer(m, lr=0.0, class_weight=_val_weight())   # (the constructor broadcasts rank 0's weights)
    batch_losses = []
    for j in range(2):
        vi, vl = _val_batch(rank, j)
        batch_losses.append(float(tr.validate_step(vi.to(dev), vl.to(dev))))
    end = tr.validation_epoch_end()
    torch.cuda.synchronize()
    res["val"] = {"val_loss": end["val_loss"].cpu(), "val_miou": end["val_miou"].cpu(), "val_iou": end["val_iou"].cpu(),
                  "named": end["val_iou_named"], "batch_losses": batch_losses, "world": tr.world,
                  "accumulators_reset": int(tr.val_confmat.sum()) == 0 and float(tr.val_count) == 0.0}
    res["seconds"]["val"] = time.monotonic() - t0
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def suite(dev, tmp_path_factory):
    """Starts the pair, computes the CPU oracle while it runs, joins under a time limit.  A worker that fails or outlives the
    limit fails every test that uses this fixture, and nothing further is started on the GPU by them."""
    import ddp_cases as D
    ctx = mp.get_context("spawn")
    out_dir = str(tmp_path_factory.mktemp("ddp_suite"))
    port = _free_port()
    procs = [ctx.Process(target=_suite_worker, args=(r, port, out_dir)) for r in range(2)]
    for p in procs:
        p.start()
    oracle = {"f64": D.two_replica_step(torch.float64), "f32": D.two_replica_step(torch.float32)}
    deadline = time.monotonic() + SUITE_TIME_LIMIT
    pending = list(procs)
    failed = False
    while pending and not failed:
        left = deadline - time.monotonic()
        if left <= 0:
            break
        _wait_any([p.sentinel for p in pending], timeout=left)
        failed = any(p.exitcode not in (None, 0) for p in procs)   # one rank gone: the other would sit in its next collective
        pending = [p for p in pending if p.is_alive()]
    late = [p for p in procs if p.is_alive()]
    for p in late:
        p.kill()
        p.join()
    codes = [p.exitcode for p in procs]
    assert not late or failed, f"worker(s) still running after {SUITE_TIME_LIMIT} s, killed: exit codes {codes}"
    assert codes == [0, 0], codes
    ranks = [torch.load(os.path.join(out_dir, f"rank{r}.pt"), weights_only=False) for r in range(2)]
    print("suite seconds per rank (cumulative):", [r["seconds"] for r in ranks])
    return {"ranks": ranks, "oracle": oracle}


def test_first_step_matches_the_two_replica_oracle(suite):
    """One fp32 train_step of two ranks (different initial weights, per-rank batches 2x5x96x128, lr 0.05) against the two-replica
    CPU oracle: per-rank BatchNorm statistics, the MEAN of the two gradients, rank 0's running statistics on both ranks.

    trainer.grads / 2 is judged like every fp32 gradient here (parity_helpers.assert_as_good_as_cpu_fp32): its per-tensor errors
    against the fp64 two-replica mean, relative to those of the same step in CPU fp32, at the median / 90th percentile /
    maximum.  Measured on the MI355X, both ranks alike (they hold the same sum): 1.36x / 1.31x / 1.12x (HIP 1.04e-2 / 1.39e-2 /
    4.95e-2 against CPU fp32 7.68e-3 / 1.06e-2 / 4.44e-2), recorded as ddp_first_step_grad_vs_fp64_rank{0,1}.  Bounds
    FIRST_STEP_BOUNDS = 2.0 / 2.0 / 3.0: the whole-model bounds 1.5 / 2.0 / 3.0 were the starting point and the 90th percentile
    and the maximum sit well inside them; the median's 1.36x leaves 1.5 less room than the helper's docstring asks for (the SAME
    code reads 0.83x ... 1.57x at the median depending on which pre-activations of a batch sit on a ReLU edge, and its bounds
    keep about 0.4 above the measurement), so the median takes the helper's next documented bound, 2.0.  The exchange itself
    adds one fp32 addition per element, 6e-8 relative.  The wrong exchanges (global statistics, one rank's gradient alone, sum
    instead of mean) sit 130-165x out, at errors near 1 (test_ddp_cases_cpu.py)."""
    import ddp_cases as D
    from parity_helpers import assert_as_good_as_cpu_fp32
    o64, o32 = suite["oracle"]["f64"], suite["oracle"]["f32"]
    e_cpu = D.tensor_errs(o32["mean_grad"], o64["mean_grad"])
    cat = lambda b: torch.cat([b[k].double().flatten() for k in sorted(b)])
    for rank, res in enumerate(suite["ranks"]):
        first = res["first"]
        e_hip = D.tensor_errs(first["mean_grad"], o64["mean_grad"])
        qh, qc = D.quantiles(e_hip), D.quantiles(e_cpu)
        print(f"rank {rank}: HIP / CPU-fp32 error ratios median {qh[0] / qc[0]:.3f} p90 {qh[1] / qc[1]:.3f} max {qh[2] / qc[2]:.3f}"
              f" (HIP {qh[0]:.3e} {qh[1]:.3e} {qh[2]:.3e}; loss {first['loss']:.7f} vs fp64 {o64['loss'][rank]:.7f})")
        assert_as_good_as_cpu_fp32(e_hip, e_cpu, f"ddp_first_step_grad_vs_fp64_rank{rank}", FIRST_STEP_BOUNDS)
        assert abs(first["loss"] - o64["loss"][rank]) < 1e-4, (rank, first["loss"], o64["loss"][rank])
        # rank 0's running statistics on BOTH ranks, and not rank 1's own
        assert sorted(first["buffers"]) == sorted(o64["buffers"][0])
        for k, b in first["buffers"].items():
            assert torch.allclose(b.float(), o64["buffers"][0][k].float(), rtol=1e-4, atol=1e-5), (rank, k)
        assert not torch.allclose(cat(first["buffers"]), cat(o64["buffers"][1]), rtol=1e-4, atol=1e-5)
    assert torch.equal(suite["ranks"][0]["first"]["flat_buffers"], suite["ranks"][1]["first"]["flat_buffers"])


def test_bucket_boundaries_and_overlap_are_invisible(suite):
    """With two ranks the all-reduce is one commutative fp32 addition per element, whatever the bucket boundaries and whenever a
    bucket starts: two steps leave bit-identical weights, gradients and buffers on both ranks under min_bucket_elems 0 (seven
    buckets), the default (an intermediate number) and 1 << 30 (one bucket), each with and without overlap."""
    assert suite["ranks"][0]["buckets_first_digest"] == suite["ranks"][1]["buckets_first_digest"]   # across the ranks
    counts = {}
    for rank, res in enumerate(suite["ranks"]):
        assert set(res["buckets"]) == {(mbe, ov) for mbe in BUCKET_SIZES for ov in (True, False)}
        for (mbe, overlap), got in res["buckets"].items():
            assert got["finite"] and got["moved"] > 1e-4, (rank, mbe, overlap, got["moved"])
            assert got["same_as_first"] == {"weights": True, "grads": True, "buffers": True}, (rank, mbe, overlap, got["same_as_first"])
            sr, buckets = got["stage_ranges"], got["bucket_ranges"]
            counts[mbe] = len(buckets)
            # ready order: from the end of the buffer down to 0 without gaps, each bucket a whole number of stages
            assert buckets[0][1] == sr[6][1] and buckets[-1][0] == 0
            assert all(buckets[i][0] == buckets[i + 1][1] for i in range(len(buckets) - 1))
            begins = {b: s for s, (b, e) in enumerate(sr)}
            assert all(b in begins for b, _ in buckets)
            assert all(e - b >= mbe for b, e in buckets) or len(buckets) == 1
            # a bucket is ready when its LOWEST stage is (the backward finishes stage 6 first, stage 0 last)
            assert got["bucket_stage"] == [begins[b] for b, _ in buckets], (mbe, got["bucket_stage"], buckets)
    assert counts[BUCKET_SIZES[0]] == 7 and counts[BUCKET_SIZES[2]] == 1 and 1 < counts[BUCKET_SIZES[1]] < 7, counts
    assert suite["ranks"][0]["buckets"][(0, True)]["bucket_stage"] == [6, 5, 4, 3, 2, 1, 0]
    assert suite["ranks"][0]["buckets"][(1 << 30, True)]["bucket_stage"] == [0]


def test_one_rank_group_with_force_exchange_equals_no_exchange(suite):
    """group= and force_exchange: each rank trains on a one-rank group of its own with the whole exchange machinery running
    (stage events, comm stream, all-reduce and broadcast over one rank, lr / 1).  A sum over one rank changes nothing: bit-equal to
    the same rank's trainer without exchange; and the two ranks, no longer coupled, keep their own different weights."""
    for rank, res in enumerate(suite["ranks"]):
        for overlap, got in res["group"].items():
            ex, plain = got["exchange"], got["plain"]
            assert ex["world"] == plain["world"] == 1 and ex["exchange"] and not plain["exchange"], (rank, overlap, got)
            assert ex["src0"] == rank                       # the group's rank 0 in global numbering
            assert got["same_state"] and ex["loss"] == plain["loss"], (rank, overlap)   # weights, gradients and buffers
    assert suite["ranks"][0]["group"][True]["exchange"]["stem_weights"] != suite["ranks"][1]["group"][True]["exchange"]["stem_weights"]


def test_validation_with_two_ranks_equals_one_process_over_all_batches(suite, dev):
    """validate_step on two batches per rank, validation_epoch_end with world = 2: both ranks return the same val_loss, val_miou
    and val_iou, bit-equal to ONE process that validated all four batches from rank 0's weights — the confusion matrix is an integer
    sum and the fp64 sum of four fp32 batch losses is exact in any order."""
    import flair_amd
    import ddp_cases as D
    v0, v1 = (r["val"] for r in suite["ranks"])
    assert v0["world"] == v1["world"] == 2 and v0["accumulators_reset"] and v1["accumulators_reset"]
    m = _hip_model(D.initial_model(0).state_dict(), dev)
    tr = flair_amd.SegTrainer(m, lr=0.0, class_weight=_val_weight())
    assert tr.world == 1
    losses = [[float(tr.validate_step(*(t.to(dev) for t in _val_batch(rank, j)))) for j in range(2)] for rank in range(2)]
    end = tr.validation_epoch_end()
    assert losses[0] == v0["batch_losses"] and losses[1] == v1["batch_losses"]   # rank 1 validated with rank 0's weights
    assert losses[0] != losses[1]
    for v in (v0, v1):
        for k in ("val_loss", "val_miou", "val_iou"):
            assert torch.equal(v[k], end[k].cpu()), (k, v[k], end[k])
        assert v["named"] == end["val_iou_named"] and VAL_WEIGHT_ZERO not in v["named"] and len(v["named"]) == 12
    assert 0 < float(end["val_miou"]) < 1 and float(end["val_loss"]) > 0
