#!/usr/bin/env python3
"""Test-time augmentation at B = 32, 5 x 512 x 512, 13 classes (BATCH / SIZE / DTYPE override; default bf16): what the ensemble costs over
the forwards it is made of.

  predict   tiles/s of Unet.predict_classes(x) (no tta), of tta="flips" (4 passes) and of tta="d4" (8 passes)
  yardstick one Unet.eval_logits(x) call -- the forward every pass runs, code this feature does not touch -- and n x its time beside
            each ensemble: overhead = ensemble time / (n x eval_logits time)
  kernels   the two new launches alone: flair_d4_nchw_f32 on the batch for a flip (code 1) and for a rot90 (code 4, whose reads walk
            columns), flair_tta_accum on fp32 (B, 13, 512, 512) logits as a first, a middle and a last pass, for the same two codes;
            each with the bytes it moves and the bandwidth that makes

Windows are timed with device events around STEPS calls (default 20 for the model, 50 for the kernels) after a warm-up; WINDOWS (default 5)
windows per figure, taken in rounds over all figures so that a drift of the machine reaches each of them; median, min and max are reported.
Prints one JSON line; OUT=<file> also writes it there.  Random weights and inputs: the timing does not depend on them."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flair-1_amd"))
import flair_amd  # noqa: E402
from flair_amd import ops  # noqa: E402
from flair_amd.tta import tta_codes  # noqa: E402


def _window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def _stats(ms):
    ms = sorted(ms)
    return {"ms": round(statistics.median(ms), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def main():
    dev = torch.device("cuda:0")
    B, S, C = int(os.environ.get("BATCH", "32")), int(os.environ.get("SIZE", "512")), 13
    dt = os.environ.get("DTYPE", "bf16")
    windows = int(os.environ.get("WINDOWS", "5"))
    steps_model, steps_kernel = int(os.environ.get("STEPS", "20")), int(os.environ.get("KERNEL_STEPS", "50"))
    torch.manual_seed(2022)
    m = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=C, compute_dtype=dt).to(dev).eval()
    x = torch.randn(B, 5, S, S, device=dev)
    logits = torch.randn(B, C, S, S, device=dev)
    acc = torch.empty(B, C, S, S, device=dev)
    preds = torch.empty(B, S, S, dtype=torch.uint8, device=dev)
    prob = torch.empty(B, S, S, device=dev)

    px = B * S * S
    runs = {"predict_plain": (lambda: m.predict_classes(x, want_prob=True), steps_model, None),
            "eval_logits": (lambda: m.eval_logits(x), steps_model, None),
            "predict_tta_flips": (lambda: m.predict_classes(x, want_prob=True, tta="flips"), steps_model, None),
            "predict_tta_d4": (lambda: m.predict_classes(x, want_prob=True, tta="d4"), steps_model, None)}
    for code, name in ((1, "vflip"), (4, "rot90")):
        runs[f"d4_nchw_{name}"] = (lambda code=code: ops.d4_transform(x, code), steps_kernel, px * 5 * 8)
        runs[f"tta_accum_first_{name}"] = (lambda code=code: ops.tta_accumulate(logits, code, acc=acc, first=True, n=8), steps_kernel,
                                           px * C * 8)
        runs[f"tta_accum_middle_{name}"] = (lambda code=code: ops.tta_accumulate(logits, code, acc=acc, n=8), steps_kernel, px * C * 12)
        runs[f"tta_accum_last_{name}"] = (lambda code=code: ops.tta_accumulate(logits, code, acc=acc, preds=preds, prob=prob, n=8),
                                          steps_kernel, px * (C * 8 + 5))
    ms = {k: [] for k in runs}
    for k, (fn, _, _) in runs.items():
        for _ in range(4):   # (the fourth identical eval call is past the graph-capture threshold of small shapes)
            fn()
    for _ in range(windows):
        for k, (fn, steps, _) in runs.items():
            ms[k].append(_window(fn, steps))

    res = {"workload": f"U-Net/ResNet34 {dt}, {C} classes, batch {B} x 5 x {S} x {S}", "windows": windows,
           "steps_per_window": {"model": steps_model, "kernel": steps_kernel}, "model": {}, "kernels": {}}
    for k, (_, _, nbytes) in runs.items():
        row = _stats(ms[k])
        if nbytes is None:
            row["tiles_per_s"] = round(B / (row["ms"] / 1e3), 1)
            res["model"][k] = row
        else:
            row["bytes"] = nbytes
            row["GB_per_s"] = round(nbytes / (row["ms"] / 1e3) / 1e9, 1)
            res["kernels"][k] = row
    one = res["model"]["eval_logits"]["ms"]
    for spec in ("flips", "d4"):
        n = len(tta_codes(spec))
        row = res["model"][f"predict_tta_{spec}"]
        row["passes"] = n
        row["n_x_eval_logits_ms"] = round(n * one, 4)
        row["over_n_forwards"] = round(row["ms"] / (n * one), 4)
    line = json.dumps(res)
    print(line)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
