#!/usr/bin/env python3
"""raster_writer.write_raster on the raster zone_detect ends in: SIDE x SIDE (10 240, BASELINE config 5) generated on the device, smooth
label blobs rather than noise (CELL-pixel class cells with 1 % of the pixels redrawn, a confidence and class probabilities that vary
over hundreds of pixels), as ``output_type: argmax`` ((2, H, W) fp32, scale (1, 255)) and as 13-class ``class_prob`` ((13, H, W)
uint8), each with band and pixel interleave, tiles of TILE (512), into a file under the system temp directory.

Per case: ``write_raster`` end to end on the host clock (the call returns with the file closed), one warm-up and REPS (3) timed
calls, median and spread; the stages each alone, summed over the groups of one pass: encode and pack (device events), the pinned D2H
copy of the packed bytes (device events), the file writes (host clock, flushed); the encode of one interior stream alone next to
the encode of all streams in one launch, with the streams per CU, which says where a tail of the one-wave-per-stream kernel comes
from; for a raster of several groups the same call with ``group_bytes`` large enough for one group; the compressed size.  The
yardstick is what the tree could do with the same tensor before: ``.cpu()``, the byte conversion on the host, and one
``PIL.Image.save(compression="tiff_lzw")`` per band (PIL writes no tiled and no N-band file), YARD_REPS (1) times.
Prints one JSON line; OUT=<file> also writes it there (profiles/zone_writer.json)."""
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flair-1_amd"))
from flair_amd import ops, raster_writer  # noqa: E402

SIDE, TILE, CELL, REPS, YARD_REPS, CLASSES = (int(os.environ.get(k, v)) for k, v in (
    ("SIDE", "10240"), ("TILE", "512"), ("CELL", "32"), ("REPS", "3"), ("YARD_REPS", "1"), ("CLASSES", "13")))


def smooth_field(dev, channels, side, cell, seed):
    """(channels, side, side) fp32: a random grid of one value per ``cell`` pixels, resized bilinearly"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    grid = torch.randn(1, channels, side // cell + 2, side // cell + 2, generator=g).to(dev)
    return F.interpolate(grid, size=(side, side), mode="bilinear", align_corners=False)[0]


def argmax_raster(dev):
    g = torch.Generator(device="cpu").manual_seed(1)
    cells = torch.randint(0, 19, (SIDE // CELL + 1, SIDE // CELL + 1), generator=g).to(dev)
    cls = cells.repeat_interleave(CELL, 0).repeat_interleave(CELL, 1)[:SIDE, :SIDE].contiguous()
    salt = torch.rand(SIDE, SIDE, device=dev) < 0.01
    cls = torch.where(salt, torch.randint(0, 19, (SIDE, SIDE), device=dev), cls)
    conf = torch.sigmoid(smooth_field(dev, 1, SIDE, 8 * CELL, 2)[0] * 2)
    return torch.stack([cls.float(), conf]).contiguous()


def class_prob_raster(dev):
    out = torch.empty(CLASSES, SIDE, SIDE, dtype=torch.uint8, device=dev)
    rows = 1024
    logits = smooth_field(dev, CLASSES, SIDE, 8 * CELL, 3)
    for r in range(0, SIDE, rows):   # in row blocks: the fp32 softmax of the whole raster is 13 x 420 MB
        out[:, r:r + rows] = (torch.softmax(logits[:, r:r + rows] * 3, 0) * 255).to(torch.uint8)
    return out


def timed_calls(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return {"median_s": round(statistics.median(t), 4), "min_s": round(min(t), 4), "max_s": round(max(t), 4), "calls": reps}


def stages(raster, interleave, scale, path):
    """one pass over the groups of write_raster, every stage alone and waited for: seconds per stage, summed over the groups"""
    bands, H, W = raster.shape
    samples = bands if interleave == "pixel" else 1
    slot = ops.tiff_lzw_tile_slot_bytes(TILE, samples)
    groups = raster_writer.stream_groups(ops.tiff_tile_streams(bands, H, W, TILE, interleave), -(-W // TILE), TILE * TILE * samples,
                                         raster_writer.GROUP_BYTES)
    buf = torch.empty(max(n for _, n in groups) * slot, dtype=torch.uint8, device=raster.device)
    sc = None if scale is None else torch.tensor(scale, dtype=torch.float32).to(raster.device)
    pinned = None
    sums = {"encode": 0.0, "pack": 0.0, "d2h": 0.0, "file_write": 0.0}
    with open(path, "wb") as f:
        for first, n in groups:
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            ev[0].record()
            slots, counts = ops.tiff_lzw_encode_tiles(raster, TILE, interleave, sc, first, n)
            ev[1].record()
            ops.tiff_pack_streams(slots, counts, slot, out=buf)
            ev[2].record()
            nbytes = int(((counts.cpu().numpy().astype(np.int64) + 15) & ~15).sum())
            if pinned is None or pinned.numel() < nbytes:
                pinned = torch.empty(nbytes * 5 // 4, dtype=torch.uint8, pin_memory=True)
            ev[3].record()
            pinned[:nbytes].copy_(buf[:nbytes], non_blocking=True)
            ev[4].record()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f.write(pinned.numpy()[:nbytes])
            f.flush()
            sums["file_write"] += time.perf_counter() - t0
            sums["encode"] += ev[0].elapsed_time(ev[1]) / 1e3
            sums["pack"] += ev[1].elapsed_time(ev[2]) / 1e3
            sums["d2h"] += ev[3].elapsed_time(ev[4]) / 1e3
    return {k + "_s": round(v, 4) for k, v in sums.items()}, len(groups)


def encode_ms(raster, interleave, scale, first, n, reps=5):
    sc = None if scale is None else torch.tensor(scale, dtype=torch.float32).to(raster.device)
    ops.tiff_lzw_encode_tiles(raster, TILE, interleave, sc, first, n)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.tiff_lzw_encode_tiles(raster, TILE, interleave, sc, first, n)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(statistics.median(ms), 3)


def yardstick(raster, scale, scratch):
    """.cpu(), bytes on the host, one PIL LZW file per band: (seconds, bytes written)"""
    from PIL import Image
    Image.MAX_IMAGE_PIXELS = None
    t, size = [], 0
    for _ in range(YARD_REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = raster.cpu()
        size = 0
        for b in range(host.shape[0]):
            band = host[b]
            if scale is not None:
                band = (band * scale[b]).clamp_(0, 255).to(torch.uint8)
            p = os.path.join(scratch, f"zone_writer_yard_{b}.tif")
            Image.fromarray(band.numpy()).save(p, compression="tiff_lzw")
            size += os.path.getsize(p)
            os.unlink(p)
        t.append(time.perf_counter() - t0)
    return {"median_s": round(statistics.median(t), 3), "min_s": round(min(t), 3), "max_s": round(max(t), 3), "calls": YARD_REPS,
            "bytes": size}


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    scratch = os.environ.get("SCRATCH") or tempfile.gettempdir()
    path = os.path.join(scratch, "zone_writer_bench.tif")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    res = {"workload": f"write_raster of a {SIDE} x {SIDE} raster on the device, tiles of {TILE}, BigTIFF, group_bytes "
                       f"{raster_writer.GROUP_BYTES}, file in {scratch}", "compute_units": cus, "waves_per_cu_by_lds": 5, "cases": []}
    for kind, make, scale in (("argmax", argmax_raster, (1.0, 255.0)), (f"class_prob_{CLASSES}", class_prob_raster, None)):
        raster = make(dev)
        bands = raster.shape[0]
        raw = bands * SIDE * SIDE
        yard = yardstick(raster, scale, scratch)
        print(json.dumps({"kind": kind, "yardstick": yard}), file=sys.stderr, flush=True)
        for interleave in ("band", "pixel"):
            info = {}

            def call():
                info.update(raster_writer.write_raster(path, raster, TILE, interleave=interleave, scale=scale))
            row = {"output": kind, "bands": bands, "interleave": interleave, "raw_bytes": raw, "write_raster": timed_calls(call, REPS)}
            row.update(file_bytes=info["file_bytes"], payload_bytes=info["payload_bytes"], streams=info["streams"], groups=info["groups"],
                       ratio=round(raw / info["payload_bytes"], 2), stream_bytes=TILE * TILE * (bands if interleave == "pixel" else 1))
            row["raw_gb_per_s"] = round(raw / 1e9 / row["write_raster"]["median_s"], 2)
            row["stages_alone"], _ = stages(raster, interleave, scale, path)
            tx = -(-SIDE // TILE)
            n_first = raster_writer.stream_groups(info["streams"], tx, row["stream_bytes"], raster_writer.GROUP_BYTES)[0][1]
            row["encode_first_group_ms"] = encode_ms(raster, interleave, scale, 0, n_first)
            row["encode_first_group_streams"] = n_first
            row["encode_one_interior_stream_ms"] = encode_ms(raster, interleave, scale, (tx // 2) * tx + tx // 2, 1)
            row["streams_per_cu_first_group"] = round(n_first / cus, 2)
            if info["groups"] > 1:   # the same file with every stream in one launch: what the memory bound of group_bytes costs
                def call_one_group():
                    raster_writer.write_raster(path, raster, TILE, interleave=interleave, scale=scale, group_bytes=raw)
                row["write_raster_one_group"] = timed_calls(call_one_group, REPS)
                row["encode_all_streams_ms"] = encode_ms(raster, interleave, scale, 0, info["streams"], reps=3)
            row["yardstick_cpu_pil_per_band"] = yard
            row["yardstick_over_write_raster"] = round(yard["median_s"] / row["write_raster"]["median_s"], 2)
            res["cases"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        del raster
        torch.cuda.empty_cache()
    if os.path.exists(path):
        os.unlink(path)
    line = json.dumps(res)
    print(line)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
