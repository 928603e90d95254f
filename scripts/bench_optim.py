#!/usr/bin/env python3
"""The fused trainer's update rules (csrc/optim.hip) at bf16, B = 32, 5 x 512 x 512, 13 classes (BATCH / SIZE override).

On the U-Net's flat parameter buffer (24.4 M fp32): each kernel alone in ms and GB/s, bytes counted from the rule (12 B / element
plain SGD, 20 momentum SGD, 28 AdamW, 4 the squared norm), flair_sgd_step as the yardstick, and torch.optim over the same parameter
views in the same process (foreach, and fused=True where this torch runs it).  Then SegTrainer.train_step: plain against momentum
SGD against AdamW + clipping, alternating windows.  Every figure is the median of WINDOWS (5) windows with their min .. max, timed by
device events behind a warm-up.  Prints one JSON line; OUT=<file> also writes it there.  Random weights and labels: the timing does
not depend on them."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flair-1_amd"))
import flair_amd  # noqa: E402
from flair_amd import ops, optim  # noqa: E402


def window_ms(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def summary(ms, nbytes=None):
    ms = sorted(ms)
    out = {"ms": round(statistics.median(ms), 4), "min": round(ms[0], 4), "max": round(ms[-1], 4)}
    if nbytes is not None:
        out["GBps"] = round(nbytes / (statistics.median(ms) * 1e-3) / 1e9, 1)
    return out


def main():
    dev = torch.device("cuda:0")
    batch, size = int(os.environ.get("BATCH", "32")), int(os.environ.get("SIZE", "512"))
    windows, ksteps, tsteps = int(os.environ.get("WINDOWS", "5")), int(os.environ.get("KSTEPS", "200")), int(os.environ.get("STEPS", "40"))
    torch.manual_seed(2022)
    res = {"workload": f"U-Net/ResNet34 bf16, batch {batch} x 5 x {size} x {size}, 13 classes", "windows": windows,
           "kernel_steps_per_window": ksteps, "train_steps_per_window": tsteps}

    # ---- the kernels alone, on the flat buffer
    m = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=13, compute_dtype="bf16").to(dev).train()
    p = m.flat_parameters()
    n = p.numel()
    g = torch.randn(n, device=dev) * 1e-3
    s1, s2 = torch.zeros_like(p), torch.zeros_like(p)
    sq = torch.zeros(1, dtype=torch.float64, device=dev)
    part = torch.empty(ops.grad_sqnorm_partials(), dtype=torch.float64, device=dev)
    clip = torch.zeros(2, device=dev)
    lr = 1e-6   # the weights barely move over the thousands of timed steps
    kernels = {
        "flair_sgd_step (yardstick)": (12, lambda: ops.sgd_step_(p, g, lr)),
        "optim_sgd plain": (12, lambda: ops.optim_sgd_(p, g, None, lr)),
        "optim_sgd momentum+nesterov+wd": (20, lambda: ops.optim_sgd_(p, g, s1, lr, momentum=0.9, weight_decay=1e-4, nesterov=True)),
        "optim_sgd momentum, scaled by coef": (20, lambda: ops.optim_sgd_(p, g, s1, lr, momentum=0.9, grad_scale=0.5, coef=clip[1:2])),
        "optim_adamw": (28, lambda: ops.optim_adamw_(p, g, s1, s2, lr, step=10)),
        "optim_adamw, scaled by coef": (28, lambda: ops.optim_adamw_(p, g, s1, s2, lr, step=10, grad_scale=0.5, coef=clip[1:2])),
        "grad_sqnorm + clip_coef": (4, lambda: (ops.grad_sqnorm_(g, sq, part), ops.clip_coef_(sq, 1.0, clip[0:1], clip[1:2]))),
    }
    params = list(m.parameters())
    for q in params:
        o = (q.data_ptr() - p.data_ptr()) // 4
        q.grad = g[o:o + q.numel()].view(q.shape)
    torch_opts = {"torch SGD plain foreach": (12, lambda: torch.optim.SGD(params, lr=lr, foreach=True)),
                  "torch SGD momentum+nesterov+wd foreach": (20, lambda: torch.optim.SGD(params, lr=lr, momentum=0.9, weight_decay=1e-4, nesterov=True, foreach=True)),
                  "torch SGD momentum+nesterov+wd fused": (20, lambda: torch.optim.SGD(params, lr=lr, momentum=0.9, weight_decay=1e-4, nesterov=True, fused=True)),
                  "torch AdamW foreach": (28, lambda: torch.optim.AdamW(params, lr=lr, foreach=True)),
                  "torch AdamW fused": (28, lambda: torch.optim.AdamW(params, lr=lr, fused=True))}
    res["torch_tensors"] = len(params)
    for name, (bpe, make) in torch_opts.items():
        try:
            opt = make()
            opt.step()
            kernels[name] = (bpe, opt.step)
        except Exception as e:   # a flavour this torch build does not run is reported, not timed
            res.setdefault("not_run", {})[name] = f"{type(e).__name__}: {e}"[:200]
    times = {k: [] for k in kernels}
    for k, (_, fn) in kernels.items():
        for _ in range(10):
            fn()
    for _ in range(windows):
        for k, (_, fn) in kernels.items():
            times[k].append(window_ms(fn, ksteps))
    res["elements"] = n
    res["kernels"] = {k: dict(summary(times[k], kernels[k][0] * n), bytes_per_element=kernels[k][0]) for k in kernels}
    for q in params:
        q.grad = None
    del kernels, torch_opts, g, s1, s2, m, p, params
    torch.cuda.empty_cache()

    # ---- train_step
    x = torch.randn(batch, 5, size, size, device=dev)
    lab = torch.randint(0, 13, (batch, size, size), device=dev).to(torch.uint8)
    flavours = {"plain": {}, "sgd momentum 0.9 nesterov wd 1e-4": {"optimizer": optim.SGD(momentum=0.9, weight_decay=1e-4, nesterov=True)},
                "adamw + clip_grad_norm 1.0": {"optimizer": optim.AdamW(), "clip_grad_norm": 1.0}}
    trainers = {}
    for name, kw in flavours.items():
        mm = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=13, compute_dtype="bf16").to(dev).train()
        trainers[name] = flair_amd.SegTrainer(mm, lr=1e-4, **kw)
        for _ in range(3):
            trainers[name].train_step(x, lab)
    tms = {k: [] for k in trainers}
    for _ in range(windows):
        for k, tr in trainers.items():
            tms[k].append(window_ms(lambda: tr.train_step(x, lab), tsteps))
    res["train_step"] = {}
    for k in trainers:
        s = summary(tms[k])
        s["tiles_per_s"] = round(batch / (s["ms"] * 1e-3), 1)
        res["train_step"][k] = s
    base = res["train_step"]["plain"]["ms"]
    for k in trainers:
        res["train_step"][k]["over_plain"] = round(res["train_step"][k]["ms"] / base, 4)
    line = json.dumps(res)
    print(line)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
