#!/usr/bin/env python3
"""The head with a configurable objective (csrc/seg_loss.hip) at B = 32, 512 x 512, bf16 rows, 13 and 19 classes (BATCH / SIZE override).

On one set of buffers per class count (NHWC bf16 logits of the head's row stride, uint8 labels, gradient rows, predictions,
confusion matrix): flair_ce_head_nhwc -- the reference's criterion, the yardstick -- and flair_seg_loss_nhwc with label smoothing
0.1, focal gamma 2, Dice only and CE + Dice, each in ms, GB/s and as a share of the measured 6.29 TB/s copy rate.  Bytes are the
algorithmic ones: per pixel one label byte read and one written in the label pass, one row read, one row written, one label byte and one prediction byte
in the main pass, and one more row and label byte read by the Dice sums pass.  Then SegTrainer.train_step in tiles/s with loss=None
against each specification, one at a time, alternating windows.  Every figure is the median of WINDOWS (5) windows with their min .. max, timed by
device events behind a warm-up.  Prints one JSON line; OUT=<file> also writes it there.  Random logits and labels: the timing
depends on them only through the share of counted pixels (all of them here)."""
import ctypes
import json
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flair-1_amd"))
import flair_amd  # noqa: E402
from flair_amd import SegLoss, ops  # noqa: E402
from flair_amd import _lib as L  # noqa: E402

COPY_RATE = 6.29e12   # bytes / s, the measured device copy rate
SPECS = {"label_smoothing 0.1": SegLoss(label_smoothing=0.1), "focal gamma 2": SegLoss(focal_gamma=2.0),
         "dice only": SegLoss(ce=0.0, dice=1.0), "ce + dice": SegLoss(ce=1.0, dice=1.0)}


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
        rate = nbytes / (statistics.median(ms) * 1e-3)
        out["GBps"] = round(rate / 1e9, 1)
        out["share_of_copy_rate"] = round(rate / COPY_RATE, 3)
    return out


def operator_bench(dev, C, batch, size, windows, steps):
    l = L.lib()
    ld = 16 if C <= 16 else 32
    npix = batch * size * size
    logits = (torch.randn(npix, ld, device=dev) * 3).to(torch.bfloat16)
    labels = torch.randint(0, C, (batch, size, size), device=dev).to(torch.uint8)
    dl = torch.empty(npix, ld, dtype=torch.bfloat16, device=dev)
    preds = torch.empty(batch, size, size, dtype=torch.uint8, device=dev)
    cm = torch.zeros(C, C, dtype=torch.int64, device=dev)
    loss = torch.zeros(3, device=dev)
    ws = torch.empty(l.flair_seg_loss_workspace_bytes(batch, C, size, size) + 256, dtype=torch.uint8, device=dev)
    row = ld * 2
    main_bytes = npix * (2 + 2 * row + 2)   # label pass 1 + 1, main pass row read + row written + label + prediction

    def ce_head():
        L.check(l.flair_ce_head_nhwc(L.ptr(logits), L.DT_BF16, ld, L.ptr(labels), 0, None, batch, C, size, size, L.ptr(loss), L.ptr(dl),
                                     L.ptr(preds), None, L.ptr(cm), L.ptr(ws), L.stream()), "ce_head_nhwc")

    def seg(spec_c):
        def run():
            L.check(l.flair_seg_loss_nhwc(L.ptr(logits), L.DT_BF16, ld, L.ptr(labels), 0, None, batch, C, size, size, ctypes.byref(spec_c),
                                          L.ptr(loss), L.ptr(dl), L.ptr(preds), None, L.ptr(cm), L.ptr(ws), L.stream()), "seg_loss_nhwc")
        return run

    fns = {"flair_ce_head_nhwc (yardstick)": (main_bytes, ce_head)}
    for name, spec in SPECS.items():
        fns["flair_seg_loss_nhwc " + name] = (main_bytes + (npix * (row + 1) if spec.dice > 0 else 0), seg(ops.seg_loss_spec(spec)))
    times = {k: [] for k in fns}
    for _, fn in fns.values():
        for _ in range(5):
            fn()
    for _ in range(windows):
        for k, (_, fn) in fns.items():
            times[k].append(window_ms(fn, steps))
    out = {k: dict(summary(times[k], fns[k][0]), bytes_per_pixel=round(fns[k][0] / npix, 1)) for k in fns}
    base = out["flair_ce_head_nhwc (yardstick)"]["ms"]
    for k in out:
        out[k]["over_ce_head"] = round(out[k]["ms"] / base, 3)
    return {"row_stride": ld, "calls": out}


def trainer_bench(dev, C, batch, size, windows, steps):
    """loss=None against one specification at a time, alternating windows: two trainers alive, never more (five models with their
    B = 32 workspaces in one process slowed the last ones made by half, whatever their specification)."""
    x = torch.randn(batch, 5, size, size, device=dev)
    lab = torch.randint(0, C, (batch, size, size), device=dev).to(torch.uint8)

    def make(spec):
        m = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=C, compute_dtype="bf16").to(dev).train()
        tr = flair_amd.SegTrainer(m, lr=1e-4, loss=spec)
        for _ in range(3):
            tr.train_step(x, lab)
        return tr

    base = make(None)
    out, none_all = {}, []
    for name, spec in SPECS.items():
        tr = make(spec)
        t_none, t_spec = [], []
        for _ in range(windows):
            t_none.append(window_ms(lambda: base.train_step(x, lab), steps))
            t_spec.append(window_ms(lambda: tr.train_step(x, lab), steps))
        s, n = summary(t_spec), summary(t_none)
        s["tiles_per_s"] = round(batch / (s["ms"] * 1e-3), 1)
        s["none_ms_same_windows"] = n["ms"]
        s["over_none"] = round(s["ms"] / n["ms"], 4)
        out[name] = s
        none_all += t_none
        del tr
        torch.cuda.empty_cache()
    n = summary(none_all)
    n["tiles_per_s"] = round(batch / (n["ms"] * 1e-3), 1)
    n["over_none"] = 1.0
    return dict({"loss=None": n}, **out)


def main():
    dev = torch.device("cuda:0")
    batch, size = int(os.environ.get("BATCH", "32")), int(os.environ.get("SIZE", "512"))
    windows, ksteps, tsteps = int(os.environ.get("WINDOWS", "5")), int(os.environ.get("KSTEPS", "50")), int(os.environ.get("STEPS", "10"))
    classes = [int(c) for c in os.environ.get("CLASSES", "13,19").split(",")]
    torch.manual_seed(2022)
    res = {"workload": f"bf16 NHWC rows, batch {batch} x {size} x {size}", "windows": windows, "calls_per_window": ksteps,
           "train_steps_per_window": tsteps, "copy_rate_TBps": COPY_RATE / 1e12, "operator": {}, "train_step": {}}
    child = os.environ.get("BENCH_LOSS_TRAIN_C")
    if child:   # one class count's train_step section, in a process of its own (below)
        print(json.dumps(trainer_bench(dev, int(child), batch, size, windows, tsteps)))
        return
    for C in classes:
        res["operator"][f"C{C}"] = operator_bench(dev, C, batch, size, windows, ksteps)
        torch.cuda.empty_cache()
    if os.environ.get("TRAIN", "1") != "0":
        # a fresh process per class count: a trainer made after gigabytes of earlier buffers were freed in the same process has been
        # seen to run its whole step at 18 ms instead of 11, loss=None included, and to stay there
        for C in classes:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, BENCH_LOSS_TRAIN_C=str(C)),
                               capture_output=True, text=True, check=True)
            res["train_step"][f"C{C}"] = json.loads(r.stdout.strip().splitlines()[-1])
    line = json.dumps(res)
    print(line)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
