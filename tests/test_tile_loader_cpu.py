"""CPU suite of the tile loader (flair_amd/tile_loader.py, tiff_chunks_to_batch_kernel in csrc/tiff_read.hip): the kernel's contract
restated in numpy against the single-raster restatement, the plan of a mixed batch, the refusals that come before any device work,
the index sequence of an epoch, and the declaration of the new symbol.  Byte and integer work: every assertion is exact."""
import os
import re

import numpy as np
import pytest
import torch

import raster_reader_cases as rc
import tile_loader_cases as lc
from flair_amd import raster_reader as rr
from flair_amd import tile_loader as tl
from flair_amd.tiff_staging import GROUP_BYTES, stream_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _four():
    """tiled planar-2 LZW, pixel strips with predictor 2, stored strips, a BigTIFF MM file"""
    files, rasters = zip(*(lc.image_file(i) for i in range(4)))
    return list(files), np.stack(rasters)


# ------------------------------------------------------------------------------------------------------------ the kernel, restated
def test_batch_restatement_agrees_with_planes_ref_file_by_file():
    files, rasters = _four()
    files, rasters = files[:3], rasters[:3]
    plan = tl.plan_batch(files)
    slots = [s for data, lay in zip(files, plan.layouts) for s in lc.host_slots(data, lay)]
    assert len({(lay.tiled, lay.planar, lay.predictor, lay.compression) for lay in plan.layouts}) == 3
    status = np.zeros(plan.n_chunks, np.int32)
    status[[3, plan.n_chunks - 1]] = 4
    got = lc.batch_ref(slots, plan.table, status, np.full((15, 32, 32), lc.FILL, np.uint8), plan.slot)
    want = np.full((3, 5, 32, 32), lc.FILL, np.uint8)
    for i, lay in enumerate(plan.layouts):
        sl = slice(plan.first[i], plan.first[i] + lay.n_chunks)
        rc.planes_ref(slots[sl], lay.chunk_table(), status[sl], lay.samples, lay.predictor, want[i])
    assert np.array_equal(got.reshape(3, 5, 32, 32), want)
    assert (got == lc.FILL).any() and (want != rasters).any()            # the two failed chunks left their rectangles
    clean = lc.batch_ref(slots, plan.table, 0 * status, np.full((15, 32, 32), lc.FILL, np.uint8), plan.slot)
    assert np.array_equal(clean.reshape(3, 5, 32, 32), rasters)


def test_the_kernel_table_reaches_every_rule():
    scratch, table, status, max_rows = lc.kernel_launch()
    want = lc.batch_ref(list(scratch), table, status, np.full(lc.KERNEL_SHAPE, lc.FILL, np.uint8), lc.KERNEL_SLOT)
    good = [i for i, (r, st) in enumerate(lc.KERNEL_ROWS) if st == 0 and min(r[:2]) >= 0 and min(r[2:4]) >= 1 and r[5] >= 1 and
            0 <= r[4] <= 9 - r[5] and r[6] in (1, 2) and r[2] * r[3] * r[5] <= lc.KERNEL_SLOT]
    assert good == list(range(10)) + [len(lc.KERNEL_ROWS) - 1] and max_rows == 37
    assert {table[i, 2] for i in good} >= {16, 53, 64, 65, 130} and {table[i, 5] for i in good} == {1, 3}
    # no two good chunks write one byte: the launch's result does not depend on the order of its blocks
    hits = np.zeros(lc.KERNEL_SHAPE, np.int32)
    for i in good:
        x0, y0, w, h, p0, s = table[i, :6]
        hits[p0:p0 + s, y0:y0 + h, x0:x0 + w] += 1
    assert hits.max() == 1 and ((hits == 0) == (want == lc.FILL)).mean() > 0.99   # (a written byte may equal the fill by chance)
    assert (want[:, :, -1] != lc.FILL).any() and (want[:, -1, :] != lc.FILL).any()   # clipped chunks reach the last column and row


# ------------------------------------------------------------------------------------------------------------------ plan_batch
def test_plan_of_a_mixed_batch():
    files, _ = _four()
    plan = tl.plan_batch(files)
    lays = [rr.raster_layout(f) for f in files]
    assert [(x.tiled, x.planar, x.predictor, x.compression, x.bigtiff, x.order) for x in lays] == [
        (True, 2, 1, 5, False, "<"), (False, 1, 2, 5, False, "<"), (False, 1, 1, 1, False, "<"), (False, 2, 1, 5, True, ">")]
    assert (plan.bands, plan.H, plan.W) == (5, 32, 32)
    counts = [x.n_chunks for x in lays]
    assert counts == [20, 5, 7, 20] and plan.n_chunks == sum(counts)
    assert plan.first.tolist() == [0, 20, 25, 32] and plan.owner.tolist() == sum(([i] * c for i, c in enumerate(counts)), [])
    bases, at = [], 0
    for f in files:
        bases.append(at)
        at += -(-len(f) // 16) * 16
    assert plan.bases.tolist() == bases and plan.src_bytes == at
    assert plan.table.dtype == np.int32 and plan.table.shape == (52, 8) and plan.src_off.dtype == np.int64
    for i, lay in enumerate(lays):
        sl = slice(plan.first[i], plan.first[i] + lay.n_chunks)
        t5 = lay.chunk_table()
        assert np.array_equal(plan.table[sl, :4], t5[:, :4])
        assert np.array_equal(plan.table[sl, 4], i * 5 + t5[:, 4])                      # plane0 = b * bands + band0
        assert (plan.table[sl, 5] == lay.samples).all() and (plan.table[sl, 6] == lay.predictor).all() and not plan.table[sl, 7].any()
        assert np.array_equal(plan.src_off[sl], bases[i] + lay.offsets) and np.array_equal(plan.src_len[sl], lay.counts)
        assert np.array_equal(plan.dst_len[sl], t5[:, 2] * t5[:, 3] * lay.samples)
        assert (plan.mode[sl] == (1 if lay.compression == 5 else 0)).all()
        for j in range(lay.n_chunks):   # the source offsets point at the chunk's own bytes in the concatenated buffer
            o = int(plan.src_off[sl][j]) - bases[i]
            assert o == lay.offsets[j] and o + lay.counts[j] <= len(files[i])
    assert plan.slot == 1152 == max(x.slot_bytes for x in lays) and plan.slot % rr.FLUSH_BLOCK == 0   # 32 x 7 x 5 = 1 120, rounded up
    assert plan.max_rows == 16
    assert plan.groups == [(0, 52)] == stream_groups(52, 1, 1152, GROUP_BYTES)
    small = tl.plan_batch(files, group_bytes=4096)
    assert small.groups == [(f, min(3, 52 - f)) for f in range(0, 52, 3)]
    assert sorted(c for f, n in small.groups for c in range(f, f + n)) == list(range(52))
    assert np.array_equal(small.table, plan.table) and small.slot == plan.slot
    assert tl.plan_batch(files, group_bytes=1).groups == [(c, 1) for c in range(52)]
    # masks: plane0 = b, one sample
    _, _, msk_bytes, _ = lc.tile_set(5)
    img_plan, msk_plan = tl.plan_tiles(lc.tile_set(5)[0], msk_bytes)
    assert (msk_plan.bands, msk_plan.H, msk_plan.W) == (1, 32, 32) and (msk_plan.table[:, 5] == 1).all()
    assert np.array_equal(msk_plan.table[:, 4], msk_plan.owner) and img_plan.slot == 5120      # one_strip: 32 x 32 x 5


def test_read_plan_is_what_it_was():
    """raster_reader's plan of a single file, whose slot now comes from the layout"""
    data, _ = rc.accepted_files()["tiles_16x32_pixel_pred2"]
    lay = rr.raster_layout(data)
    groups, slot, src_off, reads = rr.read_plan(lay, 3 * 2560)
    assert slot == 2560 == lay.slot_bytes and groups == [(0, 3), (3, 3), (6, 2)] and len(reads) == 3 and len(src_off) == 8
    table, src_len, dst_len, mode = lay.decode_tables()
    assert np.array_equal(table, lay.chunk_table()) and (dst_len == 16 * 32 * 5).all() and (mode == 1).all()
    assert np.array_equal(src_len, lay.counts) and src_len.dtype == dst_len.dtype == mode.dtype == np.int32


# ------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_come_before_any_device_work():
    files, _ = _four()
    deflate = rc.refused_files()["deflate"][0]
    with pytest.raises(rr.UnsupportedRaster, match=r"file 2: .*Compression"):
        tl.plan_batch(files[:2] + [deflate] + files[2:])
    with pytest.raises(rr.UnsupportedRaster, match=r"'b/IMG_2\.tif': .*Compression"):
        tl.plan_batch(files[:2] + [deflate], names=["a/IMG_0.tif", "a/IMG_1.tif", "b/IMG_2.tif"])
    with pytest.raises(rr.UnsupportedRaster, match="file 1: not a TIFF"):
        tl.plan_batch([files[0], b"II*"])
    other, _ = lc.image_file(1, 40, 56)
    with pytest.raises(ValueError, match=r"file 3 is 5 x 40 x 56") as e:
        tl.plan_batch(files[:3] + [other])
    assert not isinstance(e.value, rr.UnsupportedRaster)
    with pytest.raises(ValueError, match=r"'IMG_9\.tif' is 5 x 40 x 56"):
        tl.plan_batch([files[0], other], names=["IMG_0.tif", "IMG_9.tif"])
    # masks: a single band of the images' H x W
    imgs, _, msks, _ = lc.tile_set(3)
    two_bands = rc.build_tiff(np.concatenate([lc.mask_raster(0), lc.mask_raster(1)]), rows_per_strip=8)
    with pytest.raises(ValueError, match=r"'MSK_0\.tif' is 2 x 32 x 32") as e:
        tl.plan_tiles(imgs, [two_bands] + msks[1:], msk_names=["MSK_0.tif", "MSK_1.tif", "MSK_2.tif"])
    assert not isinstance(e.value, rr.UnsupportedRaster)
    with pytest.raises(ValueError, match=r"file 1 is 1 x 40 x 56"):
        tl.plan_tiles(imgs, [msks[0], lc.mask_file(1, 40, 56)[0], msks[2]])
    with pytest.raises(ValueError, match="2 masks for 3 images"):
        tl.plan_tiles(imgs, msks[:2])
    with pytest.raises(RuntimeError, match="HIP device"):
        tl.begin_read_tiles(["nowhere.tif"], None, "cpu")


# ---------------------------------------------------------------------------------------------------------------- epoch_batches
def test_epoch_batches():
    g = lambda: torch.Generator().manual_seed(7)   # noqa: E731
    a, b = tl.epoch_batches(14, 4, True, False, g()), tl.epoch_batches(14, 4, True, False, g())
    assert a == b and a != tl.epoch_batches(14, 4, True, False, torch.Generator().manual_seed(8))
    assert sorted(i for batch in a for i in batch) == list(range(14)) and [len(x) for x in a] == [4, 4, 4, 2]
    dropped = tl.epoch_batches(14, 4, True, True, g())
    assert dropped == a[:3]
    assert tl.epoch_batches(14, 4, False, True) == [[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]]
    assert tl.epoch_batches(14, 4, False, False)[-1] == [12, 13] and len(tl.epoch_batches(14, 4, False, False)) == 4
    assert tl.epoch_batches(12, 4, False, True) == tl.epoch_batches(12, 4, False, False) and tl.epoch_batches(0, 4, True, True) == []
    one = torch.Generator().manual_seed(7)        # a second epoch from one generator is another order
    assert tl.epoch_batches(14, 4, True, False, one) != tl.epoch_batches(14, 4, True, False, one)
    with pytest.raises(ValueError):
        tl.epoch_batches(14, 0, False, False)


def test_loader_lengths_and_settings_of_the_splits():
    files = {"IMG": [f"IMG_{i}.tif" for i in range(14)], "MSK": [f"MSK_{i}.tif" for i in range(14)], "MTD": [[0.5] * 45] * 14}
    config = {"batch_size": 4, "channels": [1, 2, 3, 4, 5], "classes": {i + 1: [1, str(i)] for i in range(13)}, "norm_type": "scaling",
              "norm_means": [], "norm_stds": [], "use_augmentation": True, "use_metadata": True, "num_workers": 1}
    train = tl.TileLoader.from_config(config, files, "train", device="cpu")
    assert (train.batch_size, train.shuffle, train.drop_last, len(train)) == (4, True, True, 3)
    assert train.feed.use_augmentations and train.msks is not None and tuple(train.mtd.shape) == (14, 45) and train.mtd.dtype == torch.float32
    val = tl.TileLoader.from_config(config, files, "val", device="cpu")
    assert (val.batch_size, val.shuffle, val.drop_last, len(val)) == (4, False, True, 3) and not val.feed.use_augmentations
    pred = tl.TileLoader.from_config(config, files, "predict", device="cpu")
    assert (pred.batch_size, pred.shuffle, pred.drop_last, len(pred)) == (1, False, False, 14) and pred.msks is None
    plain = tl.TileLoader.from_config({**config, "use_metadata": False}, files, "val", device="cpu")
    assert plain.mtd is None
    assert len(tl.TileLoader(files, None, batch_size=4)) == 4 and len(tl.TileLoader(files, None, batch_size=4, drop_last=True)) == 3
    with pytest.raises(ValueError):
        tl.TileLoader.from_config(config, files, "test")
    with pytest.raises(ValueError, match="13 masks"):
        tl.TileLoader({"IMG": files["IMG"], "MSK": files["MSK"][:13]}, None)


# ----------------------------------------------------------------------------------------------------------------- declarations
def test_new_symbol_is_declared_and_bound():
    import ctypes as C
    from flair_amd import _lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flair_hip.h")).read(), flags=re.S)
    kinds = {"int": C.c_int, "long": C.c_long}
    name = "flair_tiff_chunks_to_batch"
    m = re.search(r"\b(int|long)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/flair_hip.h"
    res, args = L.PROTOTYPES[name]
    assert res is kinds[m.group(1)]
    params = [p.strip() for p in m.group(2).split(",")]
    assert len(params) == len(args) == 11
    for p, a in zip(params, args):
        want = C.c_void_p if "*" in p else kinds[p.split()[0]]
        assert a is want, (name, p)
    from flair_amd import ops
    assert callable(ops.tiff_chunks_to_batch)


def test_exports():
    import flair_amd
    for name in ("TileLoader", "read_tiles", "tile_loader"):
        assert name in flair_amd.__all__ and hasattr(flair_amd, name)
    assert flair_amd.tile_loader is tl and flair_amd.TileLoader is tl.TileLoader
    assert tl.READ_THREADS <= 16
    for name in ("plan_batch", "begin_read_tiles", "finish_read_tiles", "read_tiles", "epoch_batches"):
        assert callable(getattr(tl, name))
