#!/usr/bin/env python3
"""metrics() end to end with the mask TIFFs decoded on the host (PIL, one thread, one file at a time) and on the device
(flair_amd/tiff.py, tiff_lzw_decode_kernel in csrc/tiff_lzw.hip): PAIRS (2048) pairs of 512 x 512 masks of 19 classes, written once
to a scratch directory (tmpfs when there is one) in three variants, truth and prediction alike:

  pil      PIL's tiff_lzw files: 4 strips of 64 KB, the kernel's large size class
  strips   the device writer's files (ops.tiff_lzw_encode + writer.tiff_lzw_file): 32 strips of 16 rows, 8 KB, the small class
  stored   uncompressed files (Compression 1): a copy

Every pair has a mask of its own, shaped like the smooth mask of bench_writer.py (32-pixel class cells, 2 % of the pixels redrawn),
stored as class + 1; its prediction is the truth with about 5 % of the pixels redrawn.  Per variant the two modes run in alternating
windows of one process (WINDOWS = 3 each) behind one warm-up call per mode on the first 64 pairs; a window is one metrics() call on the
host clock.  Reported per variant and mode: the median pairs/s, the spread of the windows (max - min); for the device mode the split
of one pass over the files into file reads + IFD parsing (host clock, the reader pool of tiff.py) and the decode kernel alone (device
events around ops.tiff_lzw_decode on chunks of 64 pairs, tables and compressed bytes already on the device) in strips/s and decoded
GB/s; and the bytes that go up per pair in either mode.  The device mode wins a variant when its median exceeds the host mode's by
more than the larger of the two spreads.  Prints one JSON line; OUT=<file> also writes it there (profiles/metrics_lzw.json)."""
import contextlib
import io
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
from flair_amd import metrics as M  # noqa: E402
from flair_amd import ops, tiff  # noqa: E402
from flair_amd.writer import tiff_lzw_file  # noqa: E402

C, S = 19, 512
VARIANTS = ("pil", "strips", "stored")


def pair(i):
    """(truth stored as class + 1, prediction) of pair i"""
    rng = np.random.default_rng(i)
    m = np.kron(rng.integers(0, C, (17, 17)), np.ones((32, 32), dtype=np.int64))[:S, :S]
    salt = rng.random((S, S)) < 0.02
    m[salt] = rng.integers(0, C, int(salt.sum()))
    p = m.copy()
    redrawn = rng.random((S, S)) < 0.05
    p[redrawn] = rng.integers(0, C, int(redrawn.sum()))
    return (m + 1).astype(np.uint8), p.astype(np.uint8)


def write_files(root, pairs, dev, batch=32):
    """<root>/<variant>/{gt/MSK_i.tif, run/predictions/PRED_IMG_i.tif, test.csv}"""
    from PIL import Image
    for v in VARIANTS:
        os.makedirs(os.path.join(root, v, "gt"))
        os.makedirs(os.path.join(root, v, "run", "predictions"))

    def names(v, i):
        return os.path.join(root, v, "gt", f"MSK_{i:06d}.tif"), os.path.join(root, v, "run", "predictions", f"PRED_IMG_{i:06d}.tif")

    for i0 in range(0, pairs, batch):
        masks = [pair(i) for i in range(i0, min(i0 + batch, pairs))]
        flat = np.stack([m for tp in masks for m in tp])                       # truth, prediction, truth, ...
        slots, counts, _, rows = ops.tiff_lzw_encode(torch.from_numpy(flat).to(dev))
        slots, counts = slots.cpu().numpy(), counts.cpu().numpy()
        for k, tp in enumerate(masks):
            for side, mask in enumerate(tp):
                Image.fromarray(mask).save(names("pil", i0 + k)[side], compression="tiff_lzw")
                Image.fromarray(mask).save(names("stored", i0 + k)[side])
                b = 2 * k + side
                with open(names("strips", i0 + k)[side], "wb") as f:
                    f.write(tiff_lzw_file(S, S, rows, [slots[b, s, :counts[b, s]] for s in range(counts.shape[1])]))
    for v in VARIANTS:
        with open(os.path.join(root, v, "test.csv"), "w") as f:
            f.writelines(f"/data/x/img/IMG_{i:06d}.tif,{names(v, i)[0]}\n" for i in range(pairs))
    return names


def config_of(root, v, csv="test.csv"):
    return {"paths": {"test_csv": os.path.join(root, v, csv)}, "classes": {k + 1: [1, f"class{k}"] for k in range(C)}}


def window(root, v, mode, dev, csv="test.csv"):
    """one metrics() call: (seconds, confusion matrix, where the files were decoded)"""
    with contextlib.redirect_stdout(io.StringIO()):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        M.metrics(config_of(root, v, csv), os.path.join(root, v, "run", "predictions"), device=dev, decode=mode)
        dt = time.perf_counter() - t0
    return dt, np.load(os.path.join(root, v, "run", "metrics", "confmat.npy")), dict(M.metrics.last_read_stats)


def device_split(files, dev, chunk_files=128, reps=5):
    """One pass over ``files`` the way tiff.read_masks goes, stage by stage: seconds of file reads + IFD parsing on the host clock,
    and the decode kernel alone (the median of ``reps`` timings with device events per chunk, summed over the chunks)."""
    read_s = kernel_ms = 0.0
    strips = decoded = compressed = 0
    for c0 in range(0, len(files), chunk_files):
        chunk = files[c0:c0 + chunk_files]
        t0 = time.perf_counter()
        sizes = [os.stat(p).st_size for p in chunk]
        bases = np.concatenate([[0], np.cumsum([(s + 15) & ~15 for s in sizes])])
        staging, _ = tiff._staging.take_next(int(bases[-1]))
        raw = staging.numpy()
        assert all(tiff._read_pool().map(tiff._read_into, [(p, memoryview(raw[b:b + s])) for p, b, s in zip(chunk, bases, sizes)]))
        layouts = [tiff.tiff_strip_layout(raw[b:b + s]) for b, s in zip(bases, sizes)]
        read_s += time.perf_counter() - t0
        assert None not in layouts
        src_off, src_len, dst_off, dst_len, mode = [], [], [], [], []
        for k, (lay, b) in enumerate(zip(layouts, bases)):
            n = lay.rows_per_strip * lay.W
            for j, (off, cnt) in enumerate(zip(lay.offsets, lay.counts)):
                src_off.append(int(b) + off)
                src_len.append(cnt)
                dst_off.append(k * S * S + j * n)
                dst_len.append(min(n, S * S - j * n))
                mode.append(1 if lay.compression == 5 else 0)
        t64 = torch.tensor([src_off, dst_off], dtype=torch.int64).to(dev)
        t32 = torch.tensor([src_len, dst_len, mode], dtype=torch.int32).to(dev)
        src = staging[:int(bases[-1])].to(dev)
        out = torch.empty(len(chunk) * S * S, dtype=torch.uint8, device=dev)
        ms = []
        for r in range(reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _, status = ops.tiff_lzw_decode(src, t64[0], t32[0], t64[1], t32[1], t32[2], out.numel(), out=out)
            e1.record()
            torch.cuda.synchronize()
            if r:
                ms.append(e0.elapsed_time(e1))
        assert int(status.abs().sum()) == 0
        kernel_ms += statistics.median(ms)
        strips += len(mode)
        decoded += out.numel()
        compressed += sum(src_len)
    return {"files": len(files), "strips": strips, "read_and_parse_s": round(read_s, 4), "decode_kernel_ms": round(kernel_ms, 3),
            "read_and_parse_files_per_s": round(len(files) / read_s, 1),
            "kernel_strips_per_s": round(strips / (kernel_ms / 1e3), 1), "kernel_decoded_GB_per_s": round(decoded / kernel_ms / 1e6, 2),
            "decoded_bytes_per_strip": decoded // strips, "compressed_bytes_per_file": round(compressed / len(files), 1)}


def main():
    dev = torch.device("cuda:0")
    pairs, windows = (int(os.environ.get(k, v)) for k, v in (("PAIRS", "2048"), ("WINDOWS", "3")))
    scratch = os.environ.get("SCRATCH") or ("/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None)
    root = tempfile.mkdtemp(prefix="bench_metrics_", dir=scratch)
    res = {"workload": f"metrics() over {pairs} pairs of {S} x {S} masks of {C} classes, chunk_tiles 64, {windows} alternating windows "
                       f"per mode; files on {'tmpfs' if root.startswith('/dev/shm') else 'the temporary directory'}", "cases": []}
    try:
        t0 = time.perf_counter()
        names = write_files(root, pairs, dev)
        res["write_files_s"] = round(time.perf_counter() - t0, 1)
        for v in VARIANTS:
            with open(os.path.join(root, v, "test.csv")) as f, open(os.path.join(root, v, "warm.csv"), "w") as g:
                g.writelines(f.readlines()[:64])
            for mode in M.DECODE_MODES:
                window(root, v, mode, dev, "warm.csv")
            secs, cms, stats = {m: [] for m in M.DECODE_MODES}, {}, {}
            for _ in range(windows):
                for mode in M.DECODE_MODES:
                    dt, cms[mode], stats[mode] = window(root, v, mode, dev)
                    secs[mode].append(dt)
                    print(json.dumps({"variant": v, "mode": mode, "pairs_per_s": round(pairs / dt, 1)}), file=sys.stderr, flush=True)
            assert np.array_equal(cms["host"], cms["device"]) and cms["host"].sum() > 0
            assert stats["device"]["device"] == 2 * pairs, stats["device"]
            row = {"variant": v, "file_bytes_per_pair": round(sum(os.path.getsize(p) for i in range(pairs) for p in names(v, i)) / pairs, 1),
                   "uploaded_bytes_per_pair": {"host": 2 * S * S}}
            for mode in M.DECODE_MODES:
                rate = sorted(pairs / dt for dt in secs[mode])
                row[mode] = {"pairs_per_s": round(statistics.median(rate), 1), "min": round(rate[0], 1), "max": round(rate[-1], 1),
                             "spread": round(rate[-1] - rate[0], 1)}
            row["uploaded_bytes_per_pair"]["device"] = row["file_bytes_per_pair"]
            files = [p for i in range(pairs) for p in names(v, i)]
            row["device_split"] = device_split(files, dev)
            row["device_over_host"] = round(row["device"]["pairs_per_s"] / row["host"]["pairs_per_s"], 3)
            row["device_wins_beyond_spread"] = (row["device"]["pairs_per_s"] - row["host"]["pairs_per_s"]
                                                > max(row["device"]["spread"], row["host"]["spread"]))
            res["cases"].append(row)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
