#!/usr/bin/env python3
"""SegTrainer.validate_step at B = 32, 5 x 512 x 512 (BATCH / SIZE override): tiles/s for bf16 with 13 and 19 classes and fp32 with
13, each with the per-pixel head in the head convolution's epilogue (FLAIR_HEAD_CE=1) and with the head convolution + ce_head
fallback (FLAIR_HEAD_CE=0).  The two settings are timed in one process, alternating, in both orders (1, 0, 0, 1, ...); every
window is STEPS steps (default 150: half a second in bf16, 2.7 s in fp32) behind a warm-up of both settings, timed by device events.  Per case: the median tiles/s of each setting, the
spread of its windows (min .. max), the ratio of the medians, and whether the fused flavour is slower beyond that spread.  Prints
one JSON line; OUT=<file> also writes it there.  Random weights and labels: the timing does not depend on them.

--metadata: BASELINE config 4 instead (19 classes, MetadataMLP, the YAML class weights), bf16 and fp32: predict at B = 32 and B = 1
(segmentation_task_predict.predict_step) and validation at B = 32, each with the metadata add inside the single native forward
(FLAIR_META_FUSE=1: predict_step -> FLAIR_ModelFactory.predict_classes, SegTrainer.validate_step(img, labels, mtd)) and on the
three-call split path (FLAIR_META_FUSE=0: encoder, add, decoder, head to fp32 NCHW logits, then flair_softmax_argmax / flair_ce_head
on them — what predict_step and validation_step ran before).  Same alternating windows, same JSON fields (fused / split)."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flair-1_amd"))
import flair_amd  # noqa: E402
from flair_amd import _lib as L  # noqa: E402


def window_ms(tr, x, lab, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        tr.validate_step(x, lab)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


CLASS_WEIGHTS_19 = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1, 0]   # the reference's YAML, 19 classes


def _window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main_metadata():
    from flair_amd import ops
    dev = torch.device("cuda:0")
    batch = int(os.environ.get("BATCH", "32"))
    warmup, pairs = int(os.environ.get("WARMUP", "3")), int(os.environ.get("PAIRS", "3"))
    C = 19
    cfg = {"model_framework": {"model_provider": "SegmentationModelsPytorch",
                               "SegmentationModelsPytorch": {"encoder_decoder": "resnet34_unet", "encoder_weights": None}},
           "use_metadata": True, "channels": [1, 2, 3, 4, 5], "classes": {i + 1: [w, f"class_{i + 1}"] for i, w in enumerate(CLASS_WEIGHTS_19)}}
    torch.manual_seed(2022)
    res = {"workload": "config 4 eval: U-Net/ResNet34 + MetadataMLP, 19 classes, 5 x 512 x 512 tiles", "windows_per_setting": 2 * pairs,
           "cases": []}
    slower_anywhere = False
    weight = torch.tensor(CLASS_WEIGHTS_19, dtype=torch.float32, device=dev)
    for dt in ("bf16", "f32"):
        model = flair_amd.FLAIR_ModelFactory(cfg, compute_dtype=dt).to(dev).eval()
        task = flair_amd.segmentation_task_predict(model, num_classes=C, use_metadata=True)
        tr = flair_amd.SegTrainer(model.seg_model, lr=0.0, class_weight=weight, metadata_encoder=model.enc)
        cm = torch.zeros(C, C, dtype=torch.int64, device=dev)

        def validate_split(x, lab, mtd):
            with torch.no_grad():
                ops.ce_head(model(x, mtd), lab, weight, want_dlogits=False, want_preds="u8", confmat=cm)

        for what, B in (("predict", batch), ("validate", batch), ("predict", 1)):
            steps = int(os.environ.get("STEPS", "0")) or (400 if B == 1 else (120 if dt == "bf16" else 40))
            x = torch.randn(B, 5, 512, 512, device=dev)
            mtd = torch.rand(B, 45, device=dev)
            lab = torch.randint(0, C, (B, 512, 512), device=dev).to(torch.uint8)
            if what == "predict":
                run = {1: lambda: task.predict_step({"img": x, "mtd": mtd}, 0), 0: lambda: task.predict_step({"img": x, "mtd": mtd}, 0)}
            else:
                run = {1: lambda: tr.validate_step(x, lab, mtd), 0: lambda: validate_split(x, lab, mtd)}
            ms = {1: [], 0: []}
            try:
                for mode in (1, 0):
                    os.environ["FLAIR_META_FUSE"] = str(mode)
                    for _ in range(warmup):
                        run[mode]()
                for p in range(pairs):
                    for order in ((1, 0), (0, 1)):
                        for mode in order:
                            os.environ["FLAIR_META_FUSE"] = str(mode)
                            for _ in range(3):   # (the other setting re-laid the eval arena: constants packed, graph captured again)
                                run[mode]()
                            ms[mode].append(_window(run[mode], steps))
            finally:
                os.environ.pop("FLAIR_META_FUSE", None)
            tr.validation_epoch_end()
            row = {"what": what, "dtype": dt, "batch": B, "steps_per_window": steps}
            for mode, name in ((1, "fused"), (0, "split")):
                tps = sorted(B / (t / 1e3) for t in ms[mode])
                row[name] = {"tiles_per_s": round(statistics.median(tps), 1), "min": round(tps[0], 1), "max": round(tps[-1], 1),
                             "ms_per_step": round(statistics.median(ms[mode]), 3)}
            row["fused_over_split"] = round(row["fused"]["tiles_per_s"] / row["split"]["tiles_per_s"], 4)
            row["fused_slower_beyond_spread"] = row["fused"]["max"] < row["split"]["min"]
            slower_anywhere |= row["fused_slower_beyond_spread"]
            res["cases"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            del x, mtd, lab
            torch.cuda.empty_cache()
        del tr, task, model
        torch.cuda.empty_cache()
    # the fused path is the default only if it is not slower than the split path in any case
    res["fused_default_supported"] = not slower_anywhere
    res["FLAIR_META_FUSE_default_chosen"] = 0 if slower_anywhere else 1
    line = json.dumps(res)
    print(line)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write(line + "\n")


def main():
    dev = torch.device("cuda:0")
    batch, size = int(os.environ.get("BATCH", "32")), int(os.environ.get("SIZE", "512"))
    warmup, steps, pairs = int(os.environ.get("WARMUP", "3")), int(os.environ.get("STEPS", "150")), int(os.environ.get("PAIRS", "4"))
    torch.manual_seed(2022)
    x = torch.randn(batch, 5, size, size, device=dev)
    res = {"workload": f"SegTrainer.validate_step, U-Net/ResNet34, batch {batch} x 5 x {size} x {size}", "steps_per_window": steps,
           "windows_per_setting": 2 * pairs, "cases": []}
    slower_anywhere = False
    for dt, classes in (("bf16", 13), ("bf16", 19), ("f32", 13)):
        m = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=classes, compute_dtype=dt).to(dev).eval()
        lab = torch.randint(0, classes, (batch, size, size), device=dev).to(torch.uint8)
        tr = flair_amd.SegTrainer(m, lr=0.0, class_weight=torch.linspace(0.5, 2, classes))
        ms = {1: [], 0: []}
        try:
            for mode in (1, 0):
                L.check(L.lib().flair_tune_set(b"FLAIR_HEAD_CE", mode))
                for _ in range(warmup):
                    tr.validate_step(x, lab)
            for p in range(pairs):
                for order in ((1, 0), (0, 1)):
                    for mode in order:
                        L.check(L.lib().flair_tune_set(b"FLAIR_HEAD_CE", mode))
                        ms[mode].append(window_ms(tr, x, lab, steps))
        finally:
            L.lib().flair_tune_set(b"FLAIR_HEAD_CE", 0)   # the library's default
        tr.validation_epoch_end()
        row = {"dtype": dt, "classes": classes}
        for mode, name in ((1, "fused"), (0, "fallback")):
            tps = sorted(batch / (t / 1e3) for t in ms[mode])
            row[name] = {"tiles_per_s": round(statistics.median(tps), 1), "min": round(tps[0], 1), "max": round(tps[-1], 1),
                         "ms_per_step": round(statistics.median(ms[mode]), 3)}
        row["fused_over_fallback"] = round(row["fused"]["tiles_per_s"] / row["fallback"]["tiles_per_s"], 4)
        # slower beyond the spread: even the fused flavour's best window is below the fallback's worst
        row["fused_slower_beyond_spread"] = row["fused"]["max"] < row["fallback"]["min"]
        slower_anywhere |= row["fused_slower_beyond_spread"]
        res["cases"].append(row)
        del tr, m
        torch.cuda.empty_cache()
    # the fused flavour is the default only if it is not slower than the fallback in any case
    res["fused_default_supported"] = not slower_anywhere
    res["FLAIR_HEAD_CE_default_chosen"] = 0 if slower_anywhere else 1
    line = json.dumps(res)
    print(line)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main_metadata() if "--metadata" in sys.argv[1:] else main()
