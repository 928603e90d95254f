"""Shared by the GPU parity tests (test_gpu_model.py, test_gpu_ddp.py): how a HIP fp32 gradient is judged against the fp64
oracle.  Needs no device itself."""


def grad_errs(params, truth):
    return {k: float((p.grad.detach().cpu().double() - truth[k].grad).abs().max() / (truth[k].grad.abs().max() + 1e-12))
            for k, p in params}


def assert_as_good_as_cpu_fp32(e_hip, e_cpu, name="grad_vs_fp64", mult=(1.5, 2.0, 3.0)):
    """Gradients through 46 training-mode BatchNorms + ReLUs are ill-conditioned in fp32: a pre-activation
    within rounding of 0 flips its ReLU mask, so torch-CPU fp32 itself sits ~1e-2 (relative, max-norm) from
    an fp64 run.  The bar for the HIP fp32 path is therefore 'as close to fp64 as the reference arithmetic':
    per-tensor relative max-norm errors against the fp64 oracle, HIP vs torch-CPU fp32, compared at the median, the
    90th percentile and the maximum.  The measured ratios are logged (profiles/r2_parity.json); the multipliers are
    those measurements plus margin for the run-to-run spread of WHICH pre-activations sit on a ReLU edge: whole-model
    path on 2x5x160x128 measured 1.13x / 1.20x / 1.00x (bounds 1.5 / 2.0 / 3.0), split path on 1x5x512x512 1.57x / 2.06x /
    1.15x (bounds 2.0 / 2.5 / 3.0).  Round 3 (scripts/debug_split_grad.py, profiles/r3_split_grad.txt): the difference is the
    BATCH, not the path — on the same 1x512x512 batch and weights the whole-model path reads 1.23x / 1.69x / 1.14x and the split
    path 1.37x / 1.61x / 1.13x, on the same 2x160x128 batch 0.83x / 0.60x / 0.97x and 0.85x / 0.59x / 0.97x (a layout change of
    fp32 data is exact; with 262 144 pixels per channel in ONE image the BatchNorm-backward sums cancel harder, and torch's
    blocked CPU reductions happen to lose less there than the tile-ordered sums here; with two smaller images it is the other
    way round)."""
    from oracle import parity
    q = lambda d, f: sorted(d.values())[min(len(d) - 1, int(f * len(d)))]
    entry = {"test": name, "tensors": len(e_hip),
             "median_hip": q(e_hip, 0.5), "median_cpu_fp32": q(e_cpu, 0.5),
             "p90_hip": q(e_hip, 0.9), "p90_cpu_fp32": q(e_cpu, 0.9),
             "max_hip": max(e_hip.values()), "max_cpu_fp32": max(e_cpu.values())}
    parity.record(entry)
    entry["bounds"] = list(mult)
    assert q(e_hip, 0.5) <= mult[0] * q(e_cpu, 0.5) + 1e-4, entry
    assert q(e_hip, 0.9) <= mult[1] * q(e_cpu, 0.9) + 1e-3, entry
    # the maximum is a single-tensor outlier statistic (one flipped ReLU in a small layer): loose bound only
    assert max(e_hip.values()) <= mult[2] * max(e_cpu.values()) + 2e-2, entry
