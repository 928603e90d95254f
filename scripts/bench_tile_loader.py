#!/usr/bin/env python3
"""tile_loader.TileLoader on the dataset it is for: TILES (256) synthetic tiles of SIDE x SIDE (512) x 5 bands of uint8 plus their
single-band masks, read in batches of BATCH (32) and fed through ``TileFeed``.  Two contents: smooth fields (one value per 256
pixels resized bilinearly, which LZW shrinks well) and uniform 8-bit noise (which it cannot shrink).  Two layouts: stored
pixel-interleaved strips of about 8 KB, the shape GDAL writes by default, and LZW tiles of TILE (256), band-interleaved, as
``write_raster`` writes them.  The files lie under the system temp directory and were just written, so they are read from the page
cache.

Per case: an epoch of the loader alone end to end on the host clock, one warm-up and REPS (3) timed epochs, median (min - max) in
tiles/s; the stages of one batch each alone and waited for: the file reads into pinned memory (host clock), the H2D copies, the two
decode launches, the two scatter launches and the feed (device events); ``SegTrainer.train_step`` (U-Net/ResNet34, bf16) fed by the
loader against the same number of steps on a resident synthetic batch.  The yardstick is what the tree could do before, in the same
run: ``read_raster`` per file, ``torch.stack``, ``TileFeed``, over YARD_BATCHES (2) batches.
Prints one JSON line; OUT=<file> also writes it there (profiles/tile_loader.json)."""
import json
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flair-1_amd"))
import flair_amd  # noqa: E402
from flair_amd import ops, raster_reader, raster_writer, tile_loader  # noqa: E402
from flair_amd.data_feed import TileFeed  # noqa: E402
from flair_amd.tiff_ifd import LONG, SHORT, build_ifd, entry  # noqa: E402

TILES, SIDE, TILE, BATCH, REPS, YARD_BATCHES, BANDS, CLASSES, TRAIN = (int(os.environ.get(k, v)) for k, v in (
    ("TILES", "256"), ("SIDE", "512"), ("TILE", "256"), ("BATCH", "32"), ("REPS", "3"), ("YARD_BATCHES", "2"), ("BANDS", "5"),
    ("CLASSES", "13"), ("TRAIN", "1")))


def stored_strips_file(hwc: np.ndarray) -> bytes:
    """a classic TIFF of stored pixel-interleaved strips of about 8 KB"""
    H, W, bands = hwc.shape
    rows = max(1, 8192 // (W * bands))
    strip, total = rows * W * bands, H * W * bands
    offsets = [8 + i * strip for i in range(-(-H // rows))]
    counts = [min(strip, total - i * strip) for i in range(len(offsets))]
    entries = [entry(256, LONG, (W,)), entry(257, LONG, (H,)), entry(258, SHORT, (8,) * bands), entry(259, SHORT, (1,)), entry(262, SHORT, (1,)),
               entry(273, LONG, offsets), entry(277, SHORT, (bands,)), entry(278, LONG, (rows,)), entry(279, LONG, counts), entry(284, SHORT, (1,))]
    if bands > 1:
        entries.append(entry(338, SHORT, (0,) * (bands - 1)))
    entries.append(entry(339, SHORT, (1,) * bands))
    ifd_at = 8 + total + total % 2
    return struct.pack("<2sHI", b"II", 42, ifd_at) + hwc.tobytes() + b"\0" * (total % 2) + build_ifd(entries, ifd_at, False, align=2)


def make_tiles(content, dev):
    """(TILES, BANDS, SIDE, SIDE) uint8 on the device, and raw labels 1 .. CLASSES in cells of 16 pixels"""
    g = torch.Generator(device=dev).manual_seed(3 if content == "smooth" else 4)
    if content == "smooth":
        img = torch.empty(TILES, BANDS, SIDE, SIDE, dtype=torch.uint8, device=dev)
        for i in range(0, TILES, 32):
            grid = torch.randn(min(32, TILES - i), BANDS, SIDE // 16 + 2, SIDE // 16 + 2, generator=g, device=dev)
            img[i:i + 32] = (torch.sigmoid(F.interpolate(grid, size=(SIDE, SIDE), mode="bilinear", align_corners=False) * 2) * 255).to(torch.uint8)
    else:
        img = torch.randint(0, 256, (TILES, BANDS, SIDE, SIDE), dtype=torch.uint8, device=dev, generator=g)
    cells = torch.randint(1, CLASSES + 1, (TILES, 1, SIDE // 16, SIDE // 16), generator=g, device=dev).float()
    msk = F.interpolate(cells, size=(SIDE, SIDE), mode="nearest")[:, 0].to(torch.uint8)
    return img, msk


def write_files(folder, layout, img, msk):
    os.makedirs(folder, exist_ok=True)
    ip, mp, nbytes = [], [], 0
    for i in range(img.shape[0]):
        ip.append(os.path.join(folder, f"IMG_{i:06d}.tif"))
        mp.append(os.path.join(folder, f"MSK_{i:06d}.tif"))
        if layout == "stored_strips":
            for p, a in ((ip[-1], img[i].permute(1, 2, 0).contiguous().cpu().numpy()), (mp[-1], msk[i][:, :, None].cpu().numpy())):
                with open(p, "wb") as f:
                    f.write(stored_strips_file(a))
        else:
            raster_writer.write_raster(ip[-1], img[i], TILE, interleave="band", bigtiff=False)
            raster_writer.write_raster(mp[-1], msk[i][None], TILE, bigtiff=False)
        nbytes += os.path.getsize(ip[-1]) + os.path.getsize(mp[-1])
    return ip, mp, nbytes


def rate(seconds, tiles):
    r = sorted(tiles / s for s in seconds)
    return {"tiles_per_s": round(statistics.median(r), 1), "min": round(r[0], 1), "max": round(r[-1], 1), "epochs": len(r)}


def timed_epochs(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return t


def stages(ip, mp, feed, dev):
    """one batch, every stage alone and waited for: milliseconds per stage"""
    paths = ip + mp
    sizes = [os.path.getsize(p) for p in paths]
    bases, total = [], 0
    for s in sizes:
        bases.append(total)
        total += (s + 15) & ~15
    pinned = torch.empty(total, dtype=torch.uint8, pin_memory=True)
    raw = pinned.numpy()
    views = [memoryview(raw[b:b + s]) for b, s in zip(bases, sizes)]
    t0 = time.perf_counter()
    list(tile_loader._read_pool().map(tile_loader._read_into, list(zip(paths, views))))
    ms = {"file_read": 1e3 * (time.perf_counter() - t0)}
    t0 = time.perf_counter()
    plans = tile_loader.plan_tiles(views[:len(ip)], views[len(ip):], img_names=ip, msk_names=mp)
    ms["plan"] = 1e3 * (time.perf_counter() - t0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
    tabs = [tile_loader._tables_pinned(p) for p in plans]
    ev[0].record()
    d_src = [pinned[b:b + p.src_bytes].to(dev, non_blocking=True) for b, p in zip((bases[0], bases[len(ip)]), plans)]
    d_tab = [t.to(dev, non_blocking=True) for t in tabs]
    ev[1].record()
    outs, decoded = [], []
    for plan, src, tab, lead in zip(plans, d_src, d_tab, ((len(ip), plans[0].bands), (len(ip),))):
        n = plan.n_chunks
        i32 = tab[8 * n:].view(torch.int32)
        assert len(plan.groups) == 1
        slots, st = ops.tiff_lzw_decode_chunks(src, tab[:8 * n].view(torch.int64), i32[:n], i32[n:2 * n], i32[2 * n:3 * n], plan.slot)
        decoded.append((plan, slots, st, i32[3 * n:].view(n, 8)))
        outs.append(torch.empty(*lead, plan.H, plan.W, dtype=torch.uint8, device=dev))
    ev[2].record()
    for (plan, slots, st, table), out in zip(decoded, outs):
        ops.tiff_chunks_to_batch(slots, table, st, out, max_rows=plan.max_rows)
    ev[3].record()
    feed(outs[0], outs[1])
    ev[4].record()
    torch.cuda.synchronize()
    assert all(int(st.abs().sum()) == 0 for _, _, st, _ in decoded)
    for k, name in enumerate(("h2d", "decode", "scatter", "feed")):
        ms[name] = ev[k].elapsed_time(ev[k + 1])
    return ({k + "_ms": round(v, 3) for k, v in ms.items()}, {"img_chunks": plans[0].n_chunks, "img_slot": plans[0].slot,
            "msk_chunks": plans[1].n_chunks, "msk_slot": plans[1].slot}, outs)


def yardstick(ip, mp, feed, dev):
    """read_raster per file, torch.stack, TileFeed"""
    def epoch():
        for b in range(0, len(ip), BATCH):
            img = torch.stack([raster_reader.read_raster(p, dev) for p in ip[b:b + BATCH]])
            msk = torch.stack([raster_reader.read_raster(p, dev)[0] for p in mp[b:b + BATCH]])
            feed(img, msk)
    return rate(timed_epochs(epoch, 1), len(ip))


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    root = os.path.join(os.environ.get("SCRATCH") or tempfile.gettempdir(), "flair_tile_loader_bench")
    feed = TileFeed(list(range(1, BANDS + 1)), CLASSES, "scaling")
    res = {"workload": f"TileLoader over {TILES} tiles of {SIDE} x {SIDE} x {BANDS} uint8 plus masks, batches of {BATCH}, norm 'scaling', no D4, "
                       f"files in {root} (page cache); read threads {tile_loader.READ_THREADS}",
           "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "cases": []}
    trainer = resident = None
    if TRAIN:
        model = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=BANDS, classes=CLASSES, compute_dtype="bf16").to(dev).train()
        trainer = flair_amd.SegTrainer(model, lr=1e-3)
        x = torch.randn(BATCH, BANDS, SIDE, SIDE, device=dev)
        lab = torch.randint(0, CLASSES, (BATCH, SIDE, SIDE), device=dev).to(torch.uint8)
        steps = TILES // BATCH

        def resident_epoch():
            for _ in range(steps):
                trainer.train_step(x, lab)
        resident = rate(timed_epochs(resident_epoch, REPS), steps * BATCH)
        res["train_step_resident_batch"] = resident
        print(json.dumps({"resident": resident}), file=sys.stderr, flush=True)
    try:
        for content in ("smooth", "noise"):
            img, msk = make_tiles(content, dev)
            for layout in ("stored_strips", "lzw_tiles"):
                folder = os.path.join(root, f"{content}_{layout}")
                ip, mp, nbytes = write_files(folder, layout, img, msk)
                loader = tile_loader.TileLoader({"IMG": ip, "MSK": mp}, feed, batch_size=BATCH, drop_last=True, device=dev)
                last = {}

                def loader_epoch():
                    for b in loader:
                        last["b"] = b
                row = {"content": content, "layout": layout, "file_bytes": nbytes, "raw_bytes": TILES * SIDE * SIDE * (BANDS + 1),
                       "loader_alone": rate(timed_epochs(loader_epoch, REPS), len(loader) * BATCH)}
                idx = slice((len(loader) - 1) * BATCH, len(loader) * BATCH)
                assert torch.equal(last["b"]["img"], feed(img[idx], msk[idx])["img"]) and torch.equal(last["b"]["msk"], feed(img[idx], msk[idx])["msk"])
                row["stages_alone_one_batch"], row["launch"], outs = stages(ip[:BATCH], mp[:BATCH], feed, dev)
                assert torch.equal(outs[0], img[:BATCH]) and torch.equal(outs[1], msk[:BATCH])
                del outs
                n_y = min(YARD_BATCHES * BATCH, TILES)
                row["yardstick_read_raster_per_file"] = rate_y = yardstick(ip[:n_y], mp[:n_y], feed, dev)
                row["loader_over_yardstick"] = round(row["loader_alone"]["tiles_per_s"] / rate_y["tiles_per_s"], 2)
                if trainer is not None:
                    def train_epoch():
                        for b in loader:
                            trainer.train_step(b["img"], b["msk"])
                    row["train_step_fed_by_loader"] = rate(timed_epochs(train_epoch, REPS), len(loader) * BATCH)
                    row["fed_over_resident"] = round(row["train_step_fed_by_loader"]["tiles_per_s"] / resident["tiles_per_s"], 3)
                res["cases"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                shutil.rmtree(folder, ignore_errors=True)
            del img, msk
            torch.cuda.empty_cache()
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
