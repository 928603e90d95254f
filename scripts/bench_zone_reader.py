#!/usr/bin/env python3
"""raster_reader.read_raster on the raster zone_detect starts from: SIDE x SIDE (10 240, BASELINE config 5) x 5 bands of uint8, written
by ``write_raster`` with tiles of TILE (512) in band and in pixel interleave, with two contents: smooth fields (the writer bench's
blobs: one value per 256 pixels resized bilinearly, which LZW shrinks well) and uniform 8-bit noise (which it cannot shrink: the worst
case for the bytes that cross PCIe and for the decoder's codes per byte).  The file lies under the system temp directory and was just
written, so it is read from the page cache.

Per case: ``read_raster`` end to end on the host clock, one warm-up and REPS (3) timed calls, median (min - max); the stages each
alone, summed over the groups of one pass: the file reads into pinned memory (host clock), the H2D copy, the decode and the scatter
into the planes (device events, each waited for).  The yardstick is what the tree could do before: the same raster as five single-band
tiled LZW files, each read by PIL and copied to the device (PIL opens no 5-band file), YARD_REPS (1) times, in the same run.
Prints one JSON line; OUT=<file> also writes it there (profiles/zone_reader.json)."""
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
from flair_amd import ops, raster_reader, raster_writer  # noqa: E402

SIDE, TILE, CELL, REPS, YARD_REPS, BANDS = (int(os.environ.get(k, v)) for k, v in (
    ("SIDE", "10240"), ("TILE", "512"), ("CELL", "32"), ("REPS", "3"), ("YARD_REPS", "1"), ("BANDS", "5")))


def smooth_raster(dev):
    g = torch.Generator(device="cpu").manual_seed(3)
    grid = torch.randn(1, BANDS, SIDE // (8 * CELL) + 2, SIDE // (8 * CELL) + 2, generator=g).to(dev)
    out = torch.empty(BANDS, SIDE, SIDE, dtype=torch.uint8, device=dev)
    for b in range(BANDS):   # band by band: the fp32 field of all bands is 2 GB
        out[b] = (torch.sigmoid(F.interpolate(grid[:, b:b + 1], size=(SIDE, SIDE), mode="bilinear", align_corners=False)[0, 0] * 2) * 255).to(torch.uint8)
    return out


def noise_raster(dev):
    g = torch.Generator(device=dev).manual_seed(4)
    return torch.randint(0, 256, (BANDS, SIDE, SIDE), dtype=torch.uint8, device=dev, generator=g)


def spread(t):
    return {"median_s": round(statistics.median(t), 4), "min_s": round(min(t), 4), "max_s": round(max(t), 4), "calls": len(t)}


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
    return spread(t)


def stages(path, dev):
    """one pass over the groups of read_raster, every stage alone and waited for: seconds per stage, summed over the groups"""
    with open(path, "rb") as f:
        data = f.read()
    layout = raster_reader.raster_layout(data)
    del data
    groups, slot, src_off, reads = raster_reader.read_plan(layout)
    table = layout.chunk_table()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    d_off, d_len, d_table = up(src_off), up(layout.counts.astype(np.int32)), up(table)
    d_dst = up((table[:, 2].astype(np.int64) * table[:, 3] * layout.samples).astype(np.int32))
    d_mode = torch.ones(layout.n_chunks, dtype=torch.int32, device=dev)
    planes = torch.empty(layout.bands, layout.H, layout.W, dtype=torch.uint8, device=dev)
    scratch = torch.empty(max(n for _, n in groups) * slot, dtype=torch.uint8, device=dev)
    nmax = max(nbytes for nbytes, _ in reads)
    pinned = torch.empty(nmax, dtype=torch.uint8, pin_memory=True)
    d_src = torch.empty(nmax, dtype=torch.uint8, device=dev)
    sums = {"file_read": 0.0, "h2d": 0.0, "decode": 0.0, "planes": 0.0}
    with open(path, "rb") as f:
        for (first, n), (nbytes, runs) in zip(groups, reads):
            t0 = time.perf_counter()
            raster_reader._read_runs(f, runs, pinned)
            sums["file_read"] += time.perf_counter() - t0
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            sl = slice(first, first + n)
            ev[0].record()
            d_src[:nbytes].copy_(pinned[:nbytes], non_blocking=True)
            ev[1].record()
            slots, st = ops.tiff_lzw_decode_chunks(d_src[:nbytes], d_off[sl], d_len[sl], d_dst[sl], d_mode[sl], slot, out=scratch[:n * slot])
            ev[2].record()
            ops.tiff_chunks_to_planes(slots, d_table[sl], st, planes, layout.samples, layout.predictor, max_rows=layout.chunk_h)
            ev[3].record()
            torch.cuda.synchronize()
            assert int(st.abs().sum()) == 0
            sums["h2d"] += ev[0].elapsed_time(ev[1]) / 1e3
            sums["decode"] += ev[1].elapsed_time(ev[2]) / 1e3
            sums["planes"] += ev[2].elapsed_time(ev[3]) / 1e3
    return {k + "_s": round(v, 4) for k, v in sums.items()}, len(groups), planes


def yardstick(raster, scratch):
    """the raster as one tiled LZW file per band, each read by PIL and copied to the device: (timing, bytes read)"""
    from PIL import Image
    Image.MAX_IMAGE_PIXELS = None
    paths = [os.path.join(scratch, f"zone_reader_yard_{b}.tif") for b in range(raster.shape[0])]
    for b, p in enumerate(paths):
        raster_writer.write_raster(p, raster[b:b + 1], TILE, bigtiff=False)
    t = []
    for _ in range(YARD_REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = torch.empty_like(raster)
        for b, p in enumerate(paths):
            with Image.open(p) as im:
                got[b] = torch.from_numpy(np.asarray(im)).to(raster.device)
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    assert torch.equal(got, raster)
    size = sum(os.path.getsize(p) for p in paths)
    for p in paths:
        os.unlink(p)
    return {**spread(t), "bytes": size}


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    scratch = os.environ.get("SCRATCH") or tempfile.gettempdir()
    path = os.path.join(scratch, "zone_reader_bench.tif")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    res = {"workload": f"read_raster of a {SIDE} x {SIDE} x {BANDS} uint8 raster written by write_raster, tiles of {TILE}, BigTIFF, "
                       f"group_bytes {raster_reader.GROUP_BYTES}, file in {scratch} (page cache)", "compute_units": cus,
           "decoder_window": ops.tiff_lzw_decode_chunks_window(), "cases": []}
    raw = BANDS * SIDE * SIDE
    for content, make in (("smooth", smooth_raster), ("noise", noise_raster)):
        raster = make(dev)
        yard = yardstick(raster, scratch)
        print(json.dumps({"content": content, "yardstick": yard}), file=sys.stderr, flush=True)
        for interleave in ("band", "pixel"):
            info = raster_writer.write_raster(path, raster, TILE, interleave=interleave)
            got = {}

            def call():
                got["x"] = raster_reader.read_raster(path, dev)
            row = {"content": content, "bands": BANDS, "interleave": interleave, "raw_bytes": raw, "file_bytes": info["file_bytes"],
                   "chunks": info["streams"], "chunk_bytes": TILE * TILE * (BANDS if interleave == "pixel" else 1),
                   "ratio": round(raw / info["payload_bytes"], 2), "read_raster": timed_calls(call, REPS)}
            assert torch.equal(got.pop("x"), raster)
            row["raw_gb_per_s"] = round(raw / 1e9 / row["read_raster"]["median_s"], 2)
            row["stages_alone"], row["groups"], planes = stages(path, dev)
            assert torch.equal(planes, raster)
            del planes
            row["chunks_per_cu_first_group"] = round(raster_reader.read_plan(raster_reader.raster_layout(open(path, "rb").read()))[0][0][1] / cus, 2)
            row["yardstick_pil_per_band"] = yard
            row["yardstick_over_read_raster"] = round(yard["median_s"] / row["read_raster"]["median_s"], 2)
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
