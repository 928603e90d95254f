#!/usr/bin/env python3
"""predictionwriter end to end, write_on_batch_end through flush, with the LZW encode on the host (PIL, one worker thread) and on the
device (csrc/tiff_lzw.hip): batches of BATCH (32) uint8 masks of 512 x 512 already on the device, BATCHES (200) batches per window into
a scratch directory, the two modes in alternating windows of one process (WINDOWS = 3 each) behind one warm-up batch per mode.

Two seeded masks, every tile of a batch the same mask: "smooth" (32-pixel class cells of 19 classes, 2 % of the pixels redrawn) and
"noise" (19 classes per pixel).  Per mask and mode: the median tiles/s on the host clock (flush ends a window), the spread of the
windows (max - min), the bytes written per tile; per mask the encode kernel's time from device events around it and, each alone, the
two stages behind it (the pinned D2H copy of the slots, the worker's framing + file writes of one batch); and, for scale, the
tiles/s of one Unet.predict_classes window (bf16, 19 classes, 5 x 512 x 512) on the same device.  The device mode wins a mask when its
median exceeds the host mode's by more than the larger of the two spreads.  Prints one JSON line; OUT=<file> also writes it there
(profiles/writer_lzw.json)."""
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flair-1_amd"))
import flair_amd  # noqa: E402
from flair_amd import ops  # noqa: E402
from flair_amd.writer import predictionwriter  # noqa: E402


def smooth_mask():
    rng = np.random.default_rng(0)
    m = np.kron(rng.integers(0, 19, (17, 17)), np.ones((32, 32), dtype=np.int64))[:512, :512]
    salt = rng.random((512, 512)) < 0.02
    m[salt] = rng.integers(0, 19, int(salt.sum()))
    return m.astype(np.uint8)


def noise_mask():
    return np.random.default_rng(0).integers(0, 19, (512, 512)).astype(np.uint8)


def window(mode, preds, batches, scratch):
    """one window: a fresh writer and directory; returns (tiles/s, bytes per tile)"""
    B = preds.shape[0]
    d = tempfile.mkdtemp(prefix=f"writer_{mode}_", dir=scratch)
    try:
        w = predictionwriter({"georeferencing_output": False}, d, "batch", encode=mode)
        w.write_on_batch_end(None, None, {"preds": preds, "id": [f"WARM_{j:02d}.tif" for j in range(B)]}, None, None, 0, 0)
        w.flush()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(batches):
            w.write_on_batch_end(None, None, {"preds": preds, "id": [f"IMG_{i * B + j:06d}.tif" for j in range(B)]}, None, None, i, 0)
        w.flush()
        dt = time.perf_counter() - t0
        w.close()
        nbytes = sum(e.stat().st_size for e in os.scandir(d) if e.name.startswith("PRED_IMG_"))
        return B * batches / dt, nbytes / (B * batches)
    finally:
        shutil.rmtree(d, ignore_errors=True)


def kernel_ms(preds, reps=20):
    ops.tiff_lzw_encode(preds)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.tiff_lzw_encode(preds)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def stages_ms(preds, scratch, reps=20):
    """the device mode's two stages behind the kernel, each alone: the pinned D2H copy of the slots and counts (device events) and
    the worker's framing + file writes of one batch (host clock); medians in ms per batch"""
    B, H, W = preds.shape
    slots, counts, _, rows = ops.tiff_lzw_encode(preds)
    h_slots = torch.empty(slots.shape, dtype=torch.uint8, pin_memory=True)
    h_counts = torch.empty(counts.shape, dtype=torch.int32, pin_memory=True)
    d2h, work = [], []
    d = tempfile.mkdtemp(prefix="writer_stages_", dir=scratch)
    try:
        w = predictionwriter({"georeferencing_output": False}, d, "batch", encode="device")
        for r in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            h_slots.copy_(slots, non_blocking=True)
            h_counts.copy_(counts, non_blocking=True)
            e1.record()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w._write_strips(h_slots.numpy(), h_counts.numpy(), H, W, rows, [f"IMG_{r * B + j:06d}.tif" for j in range(B)])
            t1 = time.perf_counter()
            if r:   # the first round warms both up
                d2h.append(e0.elapsed_time(e1))
                work.append((t1 - t0) * 1e3)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return statistics.median(d2h), statistics.median(work), slots.numel() + 4 * counts.numel()


def forward_tiles_per_s(dev, batch, steps):
    m = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=19, compute_dtype="bf16").to(dev).eval()
    x = torch.randn(batch, 5, 512, 512, device=dev)
    with torch.no_grad():
        for _ in range(5):
            m.predict_classes(x)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            m.predict_classes(x)
        e1.record()
        torch.cuda.synchronize()
    return batch * steps / (e0.elapsed_time(e1) / 1e3)


def main():
    dev = torch.device("cuda:0")
    batch, batches, windows = (int(os.environ.get(k, v)) for k, v in (("BATCH", "32"), ("BATCHES", "200"), ("WINDOWS", "3")))
    scratch = os.environ.get("SCRATCH") or tempfile.gettempdir()
    res = {"workload": f"predictionwriter, batches of {batch} uint8 masks of 512 x 512 on the device, {batches} batches per window, "
                       f"{windows} alternating windows per mode", "rows_per_strip": 16, "cases": []}
    for kind, mask in (("smooth", smooth_mask()), ("noise", noise_mask())):
        preds = torch.from_numpy(mask).to(dev).unsqueeze(0).repeat(batch, 1, 1).contiguous()
        tps = {"host": [], "device": []}
        size = {}
        for _ in range(windows):
            for mode in ("host", "device"):
                t, size[mode] = window(mode, preds, batches, scratch)
                tps[mode].append(t)
                print(json.dumps({"kind": kind, "mode": mode, "tiles_per_s": round(t, 1)}), file=sys.stderr, flush=True)
        row = {"mask": kind}
        for mode in ("host", "device"):
            v = sorted(tps[mode])
            row[mode] = {"tiles_per_s": round(statistics.median(v), 1), "min": round(v[0], 1), "max": round(v[-1], 1),
                         "spread": round(v[-1] - v[0], 1), "bytes_per_tile": round(size[mode], 1)}
        med, lo, hi = kernel_ms(preds)
        row["encode_kernel_ms"] = {"median": round(med, 4), "min": round(lo, 4), "max": round(hi, 4),
                                   "tiles_per_s": round(batch / (med / 1e3), 1)}
        d2h, work, d2h_bytes = stages_ms(preds, scratch)
        row["device_stages_ms_per_batch"] = {"encode_kernel": round(med, 4), "d2h_copy": round(d2h, 4), "d2h_bytes": d2h_bytes,
                                             "worker_framing_and_file_writes": round(work, 4)}
        row["device_over_host"] = round(row["device"]["tiles_per_s"] / row["host"]["tiles_per_s"], 3)
        row["device_wins_beyond_spread"] = (row["device"]["tiles_per_s"] - row["host"]["tiles_per_s"]
                                            > max(row["device"]["spread"], row["host"]["spread"]))
        res["cases"].append(row)
        del preds
    res["predict_forward_tiles_per_s"] = round(forward_tiles_per_s(dev, batch, int(os.environ.get("FWD_STEPS", "60"))), 1)
    line = json.dumps(res)
    print(line)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
