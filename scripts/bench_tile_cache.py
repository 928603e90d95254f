#!/usr/bin/env python3
"""TileLoader with a tile cache (flair_amd/tile_cache.py) on the files of ``bench_tile_loader.py``: TILES (256) synthetic tiles of
SIDE x SIDE (512) x 5 bands of uint8 plus masks, smooth and noise, as stored pixel strips and as LZW tiles of TILE (256), batches of
BATCH (32), norm 'scaling', no D4, the files just written and so in the page cache.

Per case, REPS (3) times after one pair that is not timed (it allocates the slabs and loads the kernels): ``cache.clear()``, then
epoch 1 (every item read, decoded and copied into its slot) and epoch 2 (every item fed from its slot), each on the host clock with
a device synchronise at either end; once with the loader alone and once feeding ``SegTrainer.train_step`` (U-Net/ResNet34, bf16).
Next to them, from the same run: the loader without a cache (``cache_bytes=0``, the code path of before), and ``train_step`` over
the same number of steps on a resident synthetic batch, whose spread over its repetitions is what "at the step's rate" is held to.
Rates are median (min - max) in tiles/s.  PARENT=<file> adds the JSON line that ``bench_tile_loader.py`` printed on the commit
before the cache, in the same session on the same machine.  Prints one JSON line; OUT=<file> also writes it there
(profiles/tile_cache.json)."""
import json
import os
import shutil
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_tile_loader as base  # noqa: E402  (puts flair-1_amd on the path)
import flair_amd  # noqa: E402
from flair_amd import tile_loader  # noqa: E402
from flair_amd.data_feed import TileFeed  # noqa: E402

TILES, SIDE, BATCH, REPS, BANDS, CLASSES = base.TILES, base.SIDE, base.BATCH, base.REPS, base.BANDS, base.CLASSES
CACHE_BYTES = int(float(os.environ.get("CACHE_GB", "1")) * 1e9)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def epoch_pairs(loader, consume):
    """([seconds of epoch 1], [seconds of epoch 2]) over REPS cleared caches, after one pair that is not timed"""
    def epoch():
        for b in loader:
            consume(b)
    first, second = [], []
    for rep in range(REPS + 1):
        loader.cache.clear()
        t1, t2 = timed(epoch), timed(epoch)
        s = loader.cache_stats
        assert s["hits"] == s["misses"] == s["resident"] == len(loader) * BATCH, s
        if rep:
            first.append(t1), second.append(t2)
    return first, second


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    root = os.path.join(os.environ.get("SCRATCH") or tempfile.gettempdir(), "flair_tile_cache_bench")
    feed = TileFeed(list(range(1, BANDS + 1)), CLASSES, "scaling")
    item = SIDE * SIDE * (BANDS + 1)
    res = {"workload": f"TileLoader(cache_bytes={CACHE_BYTES}) over {TILES} tiles of {SIDE} x {SIDE} x {BANDS} uint8 plus masks ({item} bytes an "
                       f"item, {TILES * item} resident), batches of {BATCH}, norm 'scaling', no D4, files in {root} (page cache)",
           "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count, "cases": []}
    model = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=BANDS, classes=CLASSES, compute_dtype="bf16").to(dev).train()
    trainer = flair_amd.SegTrainer(model, lr=1e-3)
    x = torch.randn(BATCH, BANDS, SIDE, SIDE, device=dev)
    lab = torch.randint(0, CLASSES, (BATCH, SIDE, SIDE), device=dev).to(torch.uint8)
    steps = TILES // BATCH

    def resident_epoch():
        for _ in range(steps):
            trainer.train_step(x, lab)

    def bare_step():
        return base.rate(base.timed_epochs(resident_epoch, REPS), steps * BATCH)
    res["train_step_resident_batch"] = bare = bare_step()
    print(json.dumps({"resident": bare}), file=sys.stderr, flush=True)
    step = lambda b: trainer.train_step(b["img"], b["msk"])   # noqa: E731
    try:
        for content in ("smooth", "noise"):
            img, msk = base.make_tiles(content, dev)
            for layout in ("stored_strips", "lzw_tiles"):
                folder = os.path.join(root, f"{content}_{layout}")
                ip, mp, nbytes = base.write_files(folder, layout, img, msk)
                files = {"IMG": ip, "MSK": mp}
                plain = tile_loader.TileLoader(files, feed, batch_size=BATCH, drop_last=True, device=dev)
                cached = tile_loader.TileLoader(files, feed, batch_size=BATCH, drop_last=True, device=dev, cache_bytes=CACHE_BYTES)
                n = len(cached) * BATCH
                last = {}
                keep_last = lambda b: last.__setitem__("b", b)   # noqa: E731
                row = {"content": content, "layout": layout, "file_bytes": nbytes, "raw_bytes": TILES * item}

                def plain_epoch(consume):
                    for b in plain:
                        consume(b)
                row["no_cache_alone"] = base.rate(base.timed_epochs(lambda: plain_epoch(keep_last), REPS), n)
                e1, e2 = epoch_pairs(cached, keep_last)
                row["epoch1_alone"], row["epoch2_alone"] = base.rate(e1, n), base.rate(e2, n)
                idx = slice(n - BATCH, n)      # the last batch of an epoch fed from the slots, against the feed of the pixels themselves
                want = feed(img[idx], msk[idx])
                assert torch.equal(last["b"]["img"], want["img"]) and torch.equal(last["b"]["msk"], want["msk"])
                del want
                last.clear()
                row["no_cache_feeding_train_step"] = base.rate(base.timed_epochs(lambda: plain_epoch(step), REPS), n)
                e1, e2 = epoch_pairs(cached, step)
                row["epoch1_feeding_train_step"], row["epoch2_feeding_train_step"] = base.rate(e1, n), base.rate(e2, n)
                row["cache_stats"] = cached.cache_stats
                row["epoch2_fed_over_resident"] = round(row["epoch2_feeding_train_step"]["tiles_per_s"] / bare["tiles_per_s"], 3)
                row["epoch1_fed_over_no_cache_fed"] = round(row["epoch1_feeding_train_step"]["tiles_per_s"] /
                                                            row["no_cache_feeding_train_step"]["tiles_per_s"], 3)
                res["cases"].append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
                del plain, cached
                shutil.rmtree(folder, ignore_errors=True)
            del img, msk
            torch.cuda.empty_cache()
        res["train_step_resident_batch_after"] = bare_step()      # the same measure at the end of the run: the drift over the run
    finally:
        shutil.rmtree(root, ignore_errors=True)
    if os.environ.get("PARENT"):
        with open(os.environ["PARENT"]) as f:
            res["parent_bench_tile_loader"] = json.loads(f.readline())
    line = json.dumps(res)
    print(line)
    if os.environ.get("OUT"):
        with open(os.environ["OUT"], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
