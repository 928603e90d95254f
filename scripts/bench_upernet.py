#!/usr/bin/env python3
"""UperNet-Swin-small (3 bands, 19 labels) on the HIP executor: forward time per batch of BATCH (default 32) windows of 512 x 512
in bf16 and in fp32, the per-kernel table of one bf16 batch (HIP events inside the library), and ZoneDetector windows/s on a
RASTER x RASTER (default 10 240) 3-band uint8 raster (512-pixel windows, margin 128, exact clipping, bf16).  Prints one JSON line;
OUT=<file> also writes it there.  Random weights: the timing does not depend on them."""
import ctypes as C_
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flair-1_amd"))
import flair_amd  # noqa: E402
from flair_amd import _lib as L  # noqa: E402
from flair_amd.zone_detect import ZoneDetector, tile_grid  # noqa: E402

GFLOP_PER_WINDOW = 516.0   # swin-small + UperNet head at 512 x 512 (torch.utils.flop_counter on the library's model)


def forward_ms(model, x, warmup, steps):
    for _ in range(warmup):
        model.forward_full(x)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        model.forward_full(x)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def kernel_table(model, x):
    model.forward_full(x)
    L.check(L.lib().flair_profile_start(8192))
    model.forward_full(x)
    n_k = L.lib().flair_profile_stop()
    name = C_.create_string_buffer(96)
    ms, fl, by, cnt = C_.c_double(), C_.c_double(), C_.c_double(), C_.c_int64()
    rows = []
    for i in range(n_k):
        L.lib().flair_profile_kernel(i, name, 96, C_.byref(ms), C_.byref(cnt), C_.byref(fl), C_.byref(by))
        rows.append({"kernel": name.value.decode(), "ms": round(ms.value, 4), "launches": cnt.value,
                     "tflops": round(fl.value / max(ms.value, 1e-9) / 1e9, 1), "gbps": round(by.value / max(ms.value, 1e-9) / 1e6, 1)})
    rows.sort(key=lambda r: -r["ms"])
    return rows


def main():
    dev = torch.device("cuda:0")
    batch = int(os.environ.get("BATCH", "32"))
    side = int(os.environ.get("RASTER", "10240"))
    warmup, steps = int(os.environ.get("WARMUP", "2")), int(os.environ.get("STEPS", "5"))
    torch.manual_seed(2022)
    x = torch.randn(batch, 3, 512, 512, device=dev)
    res = {"workload": f"UperNet-Swin-small, 3 bands, 19 labels, batch {batch} x 512 x 512", "gflop_per_window": GFLOP_PER_WINDOW}
    models = {}
    for dt in ("bf16", "f32"):
        m = flair_amd.UperNetForSemanticSegmentation(num_channels=3, num_labels=19, compute_dtype=dt).to(dev).eval()
        ms = forward_ms(m, x, warmup, steps if dt == "bf16" else max(1, steps // 2))
        res[f"forward_ms_{dt}"] = round(ms, 3)
        res[f"windows_per_s_{dt}"] = round(batch / ms * 1e3, 1)
        res[f"tflops_{dt}"] = round(GFLOP_PER_WINDOW * batch / ms, 1)   # GFLOP / ms = TFLOP / s
        models[dt] = m
    if os.environ.get("KERNELS", "1") == "1":
        res["kernels_one_batch_bf16"] = kernel_table(models["bf16"], x)
    del models["f32"]
    torch.cuda.empty_cache()
    if side > 0:
        cfg = {"img_pixels_detection": 512, "margin": 128, "output_type": "argmax", "n_classes": 19, "batch_size": batch,
               "channels": [1, 2, 3],
               "norma_task": [{"norm_type": "custom", "norm_means": [105.08, 110.87, 101.82], "norm_stds": [52.17, 45.38, 44]}]}
        raster = torch.randint(0, 256, (3, side, side), dtype=torch.uint8, device=dev)
        det = ZoneDetector(models["bf16"], cfg)
        n = len(tile_grid((side, side), 512, 128, det.stride))
        det.run(raster[:, :2048, :2048].contiguous())   # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        det.run(raster)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res.update({"zone_detect_raster": f"{side}x{side}x3 uint8, 512/128, exact clipping, bf16", "zone_detect_windows": n,
                    "zone_detect_seconds": round(dt, 3), "zone_detect_windows_per_s": round(n / dt, 1)})
    line = json.dumps(res)
    print(line)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
