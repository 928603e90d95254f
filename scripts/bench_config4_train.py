#!/usr/bin/env python3
"""BASELINE config 4 in training mode (19 classes with the YAML class weights, MetadataMLP, 5 bands) at B = 32 of 512 x 512 (BATCH
override), bf16 and fp32: tiles/s of one training step for

  (a) fused_metadata   SegTrainer.train_step(img, labels, mtd): the metadata add inside the one native training forward, the row
                       gradient out of the native backward, the MLP trained with the U-Net's SGD kernel;
  (b) split_autograd   what a config 4 user ran before: FLAIR_ModelFactory's training-mode forward (encoder, add, decoder, head as
                       separate native calls with fp32 NCHW tensors in between, under autograd) + FusedCrossEntropyLoss + backward +
                       torch.optim.SGD;
  (c) fused_plain      SegTrainer.train_step(img, labels) without metadata, the same 19 classes and weights, a model and trainer
                       of its own;
  (c') plain_on_a      the trainer of (a) called without mtd: the same model, workspace and buffers, so (a) against (c') is the
                       cost of the added work alone (two models of one dtype can differ by more than that: other addresses).

One process, three models of the same dtype alive, the cases timed alternately in both orders (a b c c', c' c b a, ...), every
window STEPS steps (default 40 in bf16, 12 in fp32: half a second or more) behind a warm-up of all of them, timed by device events.
Per case the median tiles/s and the spread of its windows (min .. max); a_over_b, a_over_c and a_over_plain_on_a are ratios of the
medians.  Prints one JSON
line; OUT=<file> also writes it there.  Random weights, labels and metadata: the timing does not depend on them."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flair-1_amd"))
import flair_amd  # noqa: E402

CLASS_WEIGHTS_19 = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 0]   # the reference's YAML, 19 classes
LR = 1e-3


def _window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_config4_train.py needs a HIP device: nothing is measured without one")
    dev = torch.device("cuda:0")
    B = int(os.environ.get("BATCH", "32"))
    warmup, pairs = int(os.environ.get("WARMUP", "3")), int(os.environ.get("PAIRS", "3"))
    C = 19
    cfg = {"model_framework": {"model_provider": "SegmentationModelsPytorch",
                               "SegmentationModelsPytorch": {"encoder_decoder": "resnet34_unet", "encoder_weights": None}},
           "use_metadata": True, "channels": [1, 2, 3, 4, 5], "classes": {i + 1: [w, f"class_{i + 1}"] for i, w in enumerate(CLASS_WEIGHTS_19)}}
    torch.manual_seed(2022)
    weight = torch.tensor(CLASS_WEIGHTS_19, dtype=torch.float32, device=dev)
    x = torch.randn(B, 5, 512, 512, device=dev)
    mtd = torch.rand(B, 45, device=dev)
    lab64 = torch.randint(0, C, (B, 512, 512), device=dev)
    lab8 = lab64.to(torch.uint8)
    res = {"workload": f"config 4 training step: U-Net/ResNet34 + MetadataMLP, 19 classes, batch {B} x 5 x 512 x 512",
           "windows_per_case": 2 * pairs, "cases": []}
    for dt in ("bf16", "f32"):
        steps = int(os.environ.get("STEPS", "0")) or (40 if dt == "bf16" else 12)
        # (a)
        fa = flair_amd.FLAIR_ModelFactory(cfg, compute_dtype=dt).to(dev).train()
        ta = flair_amd.SegTrainer(fa.seg_model, lr=LR, class_weight=weight, metadata_encoder=fa.enc)
        # (b)
        fb = flair_amd.FLAIR_ModelFactory(cfg, compute_dtype=dt).to(dev).train()
        crit = flair_amd.FusedCrossEntropyLoss(weight=weight).to(dev)
        opt = torch.optim.SGD(fb.parameters(), lr=LR)

        def split_step():
            opt.zero_grad(set_to_none=True)
            crit(fb(x, mtd), lab64).backward()
            opt.step()

        # (c)
        mc = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=C, compute_dtype=dt).to(dev).train()
        tc_ = flair_amd.SegTrainer(mc, lr=LR, class_weight=weight)
        run = {"fused_metadata": lambda: ta.train_step(x, lab8, mtd), "split_autograd": split_step,
               "fused_plain": lambda: tc_.train_step(x, lab8), "plain_on_a": lambda: ta.train_step(x, lab8)}
        ms = {k: [] for k in run}
        for k in run:
            for _ in range(warmup):
                run[k]()
        for _ in range(pairs):
            for order in (list(run), list(run)[::-1]):
                for k in order:
                    ms[k].append(_window(run[k], steps))
        row = {"dtype": dt, "batch": B, "steps_per_window": steps}
        for k in run:
            tps = sorted(B / (t / 1e3) for t in ms[k])
            row[k] = {"tiles_per_s": round(statistics.median(tps), 1), "min": round(tps[0], 1), "max": round(tps[-1], 1),
                      "ms_per_step": round(statistics.median(ms[k]), 3)}
        row["a_over_b"] = round(row["fused_metadata"]["tiles_per_s"] / row["split_autograd"]["tiles_per_s"], 4)
        row["a_over_c"] = round(row["fused_metadata"]["tiles_per_s"] / row["fused_plain"]["tiles_per_s"], 4)
        row["a_over_plain_on_a"] = round(row["fused_metadata"]["tiles_per_s"] / row["plain_on_a"]["tiles_per_s"], 4)
        row["a_not_slower_than_b"] = row["fused_metadata"]["tiles_per_s"] >= row["split_autograd"]["tiles_per_s"]
        row["loss_finite"] = bool(torch.isfinite(ta.loss)) and bool(torch.isfinite(tc_.loss))
        res["cases"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del ta, fa, fb, crit, opt, mc, tc_, run, split_step
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
