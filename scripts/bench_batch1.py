#!/usr/bin/env python3
"""The host-bound eval paths at batch 1: SegTrainer.predict and SegTrainer.validate_step on one 5 x 512 x 512 tile, bf16, 13
classes (CLASSES / DTYPE override) — about 1 ms per call, most of it host time in Unet._c_forward, so this is the figure a change
of the host mirror moves.  Three figures, tiles/s: predict and validate with FLAIR_EVAL_GRAPH=0 (eager, constants reused), and predict
with the HIP-graph replay (a validate forward carries the CE head and is never captured).  Per figure: WARMUP calls (default 20), then
WINDOWS windows (7) of CALLS calls (300), each timed by the host clock around a device synchronise; the median window counts, min and
max are its spread.  Prints one JSON line; OUT=<file> also writes it there.  Random weights and labels: the timing does not depend
on them."""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flair-1_amd"))
import flair_amd  # noqa: E402


def windows(fn, warmup, n, calls):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        out.append(calls / (time.perf_counter() - t0))
    return out


def main():
    dev = torch.device("cuda:0")
    classes, dt = int(os.environ.get("CLASSES", "13")), os.environ.get("DTYPE", "bf16")
    warmup, n, calls = int(os.environ.get("WARMUP", "20")), int(os.environ.get("WINDOWS", "7")), int(os.environ.get("CALLS", "300"))
    torch.manual_seed(2022)
    m = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=classes, compute_dtype=dt).to(dev).eval()
    tr = flair_amd.SegTrainer(m, lr=0.0, class_weight=torch.linspace(0.5, 2, classes))
    x = torch.randn(1, 5, 512, 512, device=dev)
    lab = torch.randint(0, classes, (1, 512, 512), device=dev).to(torch.uint8)
    res = {"workload": f"SegTrainer.predict / validate_step, U-Net/ResNet34, {dt}, {classes} classes, 1 x 5 x 512 x 512",
           "warmup": warmup, "windows": n, "calls_per_window": calls}
    old = os.environ.get("FLAIR_EVAL_GRAPH")
    try:
        for name, graph, fn in (("predict_bs1_eager", "0", lambda: tr.predict(x)),
                                ("validate_bs1_eager", "0", lambda: tr.validate_step(x, lab)),
                                ("predict_bs1_graph", "1", lambda: tr.predict(x))):
            os.environ["FLAIR_EVAL_GRAPH"] = graph
            tps = sorted(windows(fn, warmup, n, calls))
            res[name + "_tiles_per_s"] = round(statistics.median(tps), 1)
            res[name + "_spread"] = [round(tps[0], 1), round(tps[-1], 1)]
        tr.validation_epoch_end()
    finally:
        if old is None:
            os.environ.pop("FLAIR_EVAL_GRAPH", None)
        else:
            os.environ["FLAIR_EVAL_GRAPH"] = old
    line = json.dumps(res)
    print(line)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
