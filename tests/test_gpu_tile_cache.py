"""flair_feed_tiles_ptrs (feed_tiles_kernel<TilesByAddress> in csrc/feed.hip) through the C ABI, and TileLoader with a tile cache
(flair_amd/tile_cache.py) on top of it: sources in any order, repeated, unaligned and absent against oracle.data_feed and against
flair_feed_tiles on the same bytes, the return codes, and cached epochs against uncached ones, against the pixels the files held
when they were first read, with fewer slots than items, after a failed chunk and after a loop that was left early.  Byte work and
TileFeed's arithmetic that is pinned bit-exact: every assertion is exact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import tile_loader_cases as lc
from flair_amd import raster_reader as rr
from flair_amd import tile_loader as tl

pytestmark = pytest.mark.gpu

MEANS = [105.08, 110.87, 101.82, 106.38, 53.26]
STDS = [52.17, 45.38, 44, 39.69, 79.3]
CHANNELS = [4, 1, 2]
CLASSES = 19
FILL_F, FILL_L = -7.5, 201
ITEM = 32 * 32 * 6          # the bytes of one 32 x 32 x 5 tile and its mask
MODES = {"without": 0, "scaling": 1, "custom": 2}


# ------------------------------------------------------------------------------------------------------- the kernel through the C ABI
def _feed_args(mode, channels=CHANNELS):
    n = len(channels)
    return ((C.c_int * n)(*channels), n, MODES[mode], (C.c_double * n)(*MEANS[:n]), (C.c_double * n)(*STDS[:n]), CLASSES)


def _scattered(dev, H, W, seed):
    """six tiles and masks at scattered places of two larger buffers, tile 5 and mask 5 at odd addresses: (image buffer, mask buffer,
    image offsets, mask offsets, (6, 5, H, W) pixels, (6, H, W) raw labels with 0, the class count and 255 among them)"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (6, 5, H, W), dtype=np.uint8)
    msk = rng.integers(0, 25, (6, H, W), dtype=np.uint8)
    msk[:, 0, :3] = (0, CLASSES, 255)
    ti, tm = 5 * H * W, H * W
    img_off = [k * (ti + 16) + (1 if k == 5 else 0) for k in range(6)]
    msk_off = [k * (tm + 16) + (1 if k == 5 else 0) for k in range(6)]
    ibuf, mbuf = np.full(6 * (ti + 16) + 16, 0xEE, np.uint8), np.full(6 * (tm + 16) + 16, 0xEE, np.uint8)
    for k in range(6):
        ibuf[img_off[k]:img_off[k] + ti] = img[k].reshape(-1)
        mbuf[msk_off[k]:msk_off[k] + tm] = msk[k].reshape(-1)
    return torch.from_numpy(ibuf).to(dev), torch.from_numpy(mbuf).to(dev), img_off, msk_off, img, msk


def _check_sources(dev, H, W, launches):
    """``launches``: per launch the (vflip, hflip, k) of its four samples, or None for a launch without D4"""
    from flair_amd import _lib as L
    from flair_amd.data_feed import pack_d4
    from oracle import data_feed as F
    lib = L.lib()
    ibuf, mbuf, img_off, msk_off, img, msk = _scattered(dev, H, W, seed=H)
    assert ibuf.data_ptr() % 2 == 0 and mbuf.data_ptr() % 2 == 0
    tiles = [3, 0, 5, 0]             # scrambled, tile 0 twice, tile 5 at an odd address
    sel = [c - 1 for c in CHANNELS]
    B = len(tiles)
    for draws in launches:
        d4 = None if draws is None else torch.tensor([pack_d4(*d) for d in draws], dtype=torch.uint8, device=dev)
        for mode in MODES:
            for absent in (None, 2):
                ip = torch.tensor([0 if s == absent else ibuf.data_ptr() + img_off[t] for s, t in enumerate(tiles)], dtype=torch.int64, device=dev)
                mp = torch.tensor([0 if s == absent else mbuf.data_ptr() + msk_off[t] for s, t in enumerate(tiles)], dtype=torch.int64, device=dev)
                out = torch.full((B, len(CHANNELS), H, W), FILL_F, dtype=torch.float32, device=dev)
                lab = torch.full((B, H, W), FILL_L, dtype=torch.uint8, device=dev)
                assert lib.flair_feed_tiles_ptrs(L.ptr(ip), L.ptr(mp), L.ptr(d4), B, 5, H, W, *_feed_args(mode), L.ptr(out), L.ptr(lab),
                                                 L.stream()) == 0
                # the same bytes one behind the other, through the entry point that tests/test_gpu_feed.py pins
                packed_i, packed_m = torch.from_numpy(img[tiles]).to(dev), torch.from_numpy(msk[tiles]).to(dev)
                out2, lab2 = torch.empty_like(out), torch.empty_like(lab)
                assert lib.flair_feed_tiles(L.ptr(packed_i), L.ptr(packed_m), L.ptr(d4), B, 5, H, W, *_feed_args(mode), L.ptr(out2),
                                            L.ptr(lab2), L.stream()) == 0
                got_i, got_l = out.cpu().numpy(), lab.cpu().numpy()
                for s, t in enumerate(tiles):
                    if s == absent:      # an image address of 0: nothing of the sample is written
                        assert (got_i[s] == np.float32(FILL_F)).all() and (got_l[s] == FILL_L).all(), (mode, draws)
                        continue
                    v, h, k = (0, 0, 0) if draws is None else draws[s]
                    assert np.array_equal(got_i[s], F.norm_np(F.d4_np(img[t][sel], v, h, k), mode, MEANS, STDS)), (mode, draws, s)
                    assert np.array_equal(got_l[s], F.d4_np(F.labels_from_raw(msk[t], CLASSES), v, h, k)), (mode, draws, s)
                    assert torch.equal(out[s], out2[s]) and torch.equal(lab[s], lab2[s])
            # either output alone, the image one without a mask table
            only = torch.full((B, len(CHANNELS), H, W), FILL_F, dtype=torch.float32, device=dev)
            assert lib.flair_feed_tiles_ptrs(L.ptr(ip), None, L.ptr(d4), B, 5, H, W, *_feed_args(mode), L.ptr(only), None, L.stream()) == 0
            assert torch.equal(only, out)
            only_l = torch.full((B, H, W), FILL_L, dtype=torch.uint8, device=dev)
            assert lib.flair_feed_tiles_ptrs(L.ptr(ip), L.ptr(mp), L.ptr(d4), B, 5, H, W, *_feed_args(mode), None, L.ptr(only_l), L.stream()) == 0
            assert torch.equal(only_l, lab)
    assert {0, CLASSES, 255} <= set(np.unique(msk[tiles]).tolist())


def test_sources_by_address_8x12(dev):
    _check_sources(dev, 8, 12, [None])


def test_sources_by_address_16x16_every_d4_element(dev):
    from oracle import data_feed as F
    launches = [[(0, 0, 0), (1, 0, 1), (0, 1, 2), (1, 1, 3)], [(0, 0, 2), (1, 0, 3), (0, 1, 0), (1, 1, 1)]]
    probe = np.arange(16, dtype=np.int64).reshape(4, 4)
    assert len({F.d4_np(probe, *d).tobytes() for launch in launches for d in launch}) == 8      # the eight elements of D4, each once
    _check_sources(dev, 16, 16, launches)


def test_return_codes_and_refused_calls_write_nothing(dev):
    from flair_amd import _lib as L
    lib = L.lib()
    H = W = 8
    B = 4
    src = torch.zeros(B, 5, H, W, dtype=torch.uint8, device=dev)
    raw = torch.ones(B, H, W, dtype=torch.uint8, device=dev)
    ip = torch.tensor([src[b].data_ptr() for b in range(B)], dtype=torch.int64, device=dev)
    mp = torch.tensor([raw[b].data_ptr() for b in range(B)], dtype=torch.int64, device=dev)
    out = torch.full((B, 3, H, W), FILL_F, dtype=torch.float32, device=dev)
    lab = torch.full((B, H, W), FILL_L, dtype=torch.uint8, device=dev)
    d4 = torch.zeros(B, dtype=torch.uint8, device=dev)
    args = _feed_args("scaling")

    def call(ip_, mp_, out_, lab_, B_=B, bands=5, H_=H, W_=W, d4_=None, a=args):
        return lib.flair_feed_tiles_ptrs(ip_, mp_, d4_, B_, bands, H_, W_, *a, out_, lab_, L.stream())
    ok = (L.ptr(ip), L.ptr(mp), L.ptr(out), L.ptr(lab))
    assert call(None, ok[1], ok[2], ok[3]) == -1                        # no image table
    assert call(None, ok[1], None, ok[3]) == -1                         # not even for labels alone
    assert call(ok[0], None, ok[2], ok[3]) == -1                        # labels without a mask table
    assert call(ok[0], ok[1], None, None) == -1                         # nothing to write
    odd = torch.zeros(8 * B + 8, dtype=torch.uint8, device=dev)
    assert call(L.ptr(odd[4:]), ok[1], ok[2], ok[3]) == -2              # tables that are not 8-byte aligned
    assert call(ok[0], L.ptr(odd[4:]), ok[2], ok[3]) == -2
    assert call(ok[0], L.ptr(odd[1:]), ok[2], None) == -2               # an unused mask table is held to it too
    # the checks of flair_feed_tiles
    assert call(*ok, B_=0) == -2 and call(*ok, H_=0) == -2 and call(*ok, W_=6) == -2 and call(*ok, W_=0) == -2
    assert call(*ok, H_=4, W_=8, d4_=L.ptr(d4)) == -2                   # rot90 of a non-square tile
    assert call(*ok, bands=3) == -2                                     # channel 4 of 3 bands
    assert call(*ok, a=_feed_args("scaling", [0, 1, 2])) == -2          # channels start at 1
    n = 17
    assert call(*ok, a=((C.c_int * n)(*([1] * n)), n, 1, None, None, CLASSES)) == -2
    assert call(*ok, a=(args[0], 3, 3, args[3], args[4], CLASSES)) == -2                # no such normalisation
    assert call(*ok, a=(args[0], 3, 2, None, args[4], CLASSES)) == -1                   # 'custom' without means
    assert call(*ok, a=(None, 3, 1, None, None, CLASSES)) == -1                         # an image output without channels
    assert call(*ok, a=(args[0], 3, 1, None, None, 0)) == -2 and call(*ok, a=(args[0], 3, 1, None, None, 256)) == -2
    torch.cuda.synchronize()
    assert (out == FILL_F).all() and (lab == FILL_L).all()              # the refused calls wrote nothing
    assert call(*ok) == 0
    assert (out == 0).all() and (lab == 0).all()


# ---------------------------------------------------------------------------------------------------------------- the loader
@functools.lru_cache(maxsize=None)
def _expected(n, mode="scaling"):
    """what an unaugmented TileFeed([1..5], CLASSES, mode) makes of item i of tile_set(n): ((n, 5, 32, 32) fp32, (n, 32, 32) uint8)"""
    from oracle import data_feed as F
    _, img, _, msk = lc.tile_set(n)
    return (np.stack([F.norm_np(img[i], mode, MEANS, STDS) for i in range(n)]),
            np.stack([F.labels_from_raw(msk[i], CLASSES) for i in range(n)]))


def _feed(mode="scaling", **kw):
    from flair_amd.data_feed import TileFeed
    return TileFeed([1, 2, 3, 4, 5], CLASSES, mode, MEANS, STDS, **kw)


def _assert_batch(b, idx, n, mode="scaling"):
    want_img, want_msk = _expected(n, mode)
    assert b["img"].dtype == torch.float32 and b["msk"].dtype == torch.uint8
    assert np.array_equal(b["img"].cpu().numpy(), want_img[idx]) and np.array_equal(b["msk"].cpu().numpy(), want_msk[idx]), idx


def _assert_stats(loader, asked):
    s = loader.cache_stats
    assert s["hits"] + s["misses"] == asked and s["files_read"] == 2 * s["misses"] and s["resident"] <= s["capacity"], s
    return s


def test_three_cached_epochs_equal_three_uncached_ones(dev, tmp_path):
    """shuffled, augmented, with metadata: the same batches in the same order, D4 draws included, from equally seeded generators"""
    from flair_amd.data_feed import TileFeed
    n = 14
    ip, _, mp, _ = lc.write_set(tmp_path, n)
    mtd = np.random.default_rng(6).random((n, 45))
    files = {"IMG": ip, "MSK": mp, "MTD": mtd.tolist()}
    loaders = []
    for cache_bytes in (0, n * ITEM):
        g = torch.Generator().manual_seed(11)
        feed = TileFeed([3, 1, 5], CLASSES, "custom", MEANS, STDS, use_augmentations=True, generator=g)
        loaders.append(tl.TileLoader(files, feed, batch_size=4, shuffle=True, generator=g, device=dev, cache_bytes=cache_bytes))
    plain, cached = loaders
    assert plain.cache is None
    mtd32 = torch.as_tensor(mtd, dtype=torch.float32)
    for epoch in range(3):
        seen = []
        for a, b in zip(list(plain), list(cached), strict=True):
            assert sorted(a) == sorted(b) == ["img", "msk", "mtd"]
            assert torch.equal(a["img"], b["img"]) and torch.equal(a["msk"], b["msk"]) and torch.equal(a["mtd"], b["mtd"]), epoch
            seen += [int((mtd32 == row).all(1).nonzero()) for row in b["mtd"].cpu()]          # the order, read off the metadata rows
        assert sorted(seen) == list(range(n)) and len(seen) == n
        s = _assert_stats(cached, (epoch + 1) * n)
        assert s == {"hits": epoch * n, "misses": n, "files_read": 2 * n, "resident": n, "capacity": n}


def test_files_are_not_read_again(dev, tmp_path):
    """after epoch 1 every file holds other pixels; epochs 2 and 3 still yield the pixels of epoch 1 and read no file"""
    n = 12
    ip, _, mp, _ = lc.write_set(tmp_path, n)
    loader = tl.TileLoader({"IMG": ip, "MSK": mp}, _feed(), batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(3),
                           device=dev, cache_bytes=1 << 20)
    replay = torch.Generator().manual_seed(3)
    for epoch in range(3):
        order = tl.epoch_batches(n, 4, True, False, replay)
        for b, idx in zip(loader, order, strict=True):
            _assert_batch(b, idx, n)
        if epoch == 0:
            assert _assert_stats(loader, n) == {"hits": 0, "misses": n, "files_read": 2 * n, "resident": n, "capacity": n}
            img_bytes, _, msk_bytes, _ = lc.tile_set(n)
            for i in range(n):      # item i's files now hold item i + 1's pixels, in another layout
                with open(ip[i], "wb") as f:
                    f.write(img_bytes[(i + 1) % n])
                with open(mp[i], "wb") as f:
                    f.write(msk_bytes[(i + 1) % n])
    assert _assert_stats(loader, 3 * n) == {"hits": 2 * n, "misses": n, "files_read": 2 * n, "resident": n, "capacity": n}
    # clear() is the remedy: the next epoch reads the files as they are now
    loader.cache.clear()
    for b, idx in zip(loader, tl.epoch_batches(n, 4, True, False, replay), strict=True):
        _assert_batch(b, [(i + 1) % n for i in idx], n)
    assert _assert_stats(loader, n)["files_read"] == 2 * n


def test_five_slots_for_twelve_items(dev, tmp_path):
    n = 12
    ip, _, mp, _ = lc.write_set(tmp_path, n)
    loader = tl.TileLoader({"IMG": ip, "MSK": mp}, _feed("custom"), batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(8),
                           device=dev, cache_bytes=5 * ITEM + ITEM // 2)
    replay = torch.Generator().manual_seed(8)
    mixed = 0
    for epoch in range(3):
        order = tl.epoch_batches(n, 4, True, False, replay)
        resident = loader.cache.slot_of >= 0
        mixed += sum(0 < int(resident[idx].sum()) < len(idx) for idx in order)
        for b, idx in zip(loader, order, strict=True):
            _assert_batch(b, idx, n, "custom")
        s = _assert_stats(loader, (epoch + 1) * n)
        assert s["resident"] == s["capacity"] == 5
    assert mixed >= 2                   # five resident items over three batches of four: a batch of hits and misses in either later epoch
    assert s["hits"] == 2 * 5 and s["misses"] == n + 2 * 7
    assert tuple(loader.cache.img.shape) == (5, 5, 32, 32) and tuple(loader.cache.msk.shape) == (5, 32, 32)
    # below one item: no slot, no slab, every batch through the plain path
    none = tl.TileLoader({"IMG": ip, "MSK": mp}, _feed(), batch_size=4, device=dev, cache_bytes=ITEM - 1)
    for _ in range(2):
        for b, at in zip(none, range(0, n, 4), strict=True):
            _assert_batch(b, list(range(at, at + 4)), n)
    assert none.cache_stats == {"hits": 0, "misses": 2 * n, "files_read": 4 * n, "resident": 0, "capacity": 0} and none.cache.img is None


def test_a_truncated_chunk_leaves_nothing_of_its_batch_resident(dev, tmp_path):
    n = 8
    ip, _, mp, _ = lc.write_set(tmp_path, n)
    good = open(ip[5], "rb").read()
    cut = lambda i, s: s[:len(s) // 2] if i == 7 else s   # noqa: E731 - the bytes of chunk 7 run out: status 1
    with open(ip[5], "wb") as f:
        f.write(lc.image_file(0, mangle=cut)[0])          # tiled, band-interleaved: chunk 7 is the tile at (16, 16) of band 1
    loader = tl.TileLoader({"IMG": ip, "MSK": mp}, _feed(), batch_size=4, device=dev, cache_bytes=1 << 20)
    got = []
    with pytest.raises(rr.RasterDecodeError, match=r"chunk 7 \(tile at row 16, column 16, band 1\).*status 1") as e:
        for b in loader:
            got.append(b)
    assert ip[5] in str(e.value) and len(got) == 1
    _assert_batch(got[0], [0, 1, 2, 3], n)
    assert (loader.cache.slot_of >= 0).tolist() == [True] * 4 + [False] * 4 and loader.cache.free_slots == 4
    with open(ip[5], "wb") as f:
        f.write(good)
    for b, at in zip(loader, (0, 4), strict=True):
        _assert_batch(b, list(range(at, at + 4)), n)
    assert _assert_stats(loader, 2 * n) == {"hits": 4, "misses": 12, "files_read": 24, "resident": 8, "capacity": 8}
    for b, at in zip(loader, (0, 4), strict=True):
        _assert_batch(b, list(range(at, at + 4)), n)
    assert loader.cache_stats["files_read"] == 24


def test_leaving_the_loop_early_loses_no_slot(dev, tmp_path):
    n = 12
    ip, _, mp, _ = lc.write_set(tmp_path, n)
    loader = tl.TileLoader({"IMG": ip, "MSK": mp}, _feed(), batch_size=4, device=dev, cache_bytes=6 * ITEM)
    for b in loader:                    # batch 1 has been begun and holds the last two slots when the loop is left
        _assert_batch(b, [0, 1, 2, 3], n)
        break
    del b
    assert loader.cache.resident == 4 and loader.cache.free_slots == 2
    for epoch in range(2):
        for b, at in zip(loader, range(0, n, 4), strict=True):
            _assert_batch(b, list(range(at, at + 4)), n)
        s = loader.cache_stats
        assert s["resident"] == s["capacity"] == 6 and loader.cache.free_slots == 0
    assert (loader.cache.slot_of >= 0).tolist() == [True] * 6 + [False] * 6
    assert sorted(loader.cache.slot_of[:6].tolist()) == list(range(6))
    assert s["hits"] == 4 + 6 and s["hits"] + s["misses"] == 8 + 2 * n


def test_batches_held_in_a_list_stay_intact(dev, tmp_path):
    """Every batch of an epoch is produced before the first is looked at, so a batch has seen the slot copies and feeds of all later
    ones.  This is necessary, not sufficient: it cannot force the race that the stream rule excludes (slabs written and read on one
    stream only); that argument is DESIGN.md's (§10, "Tile cache")."""
    n = 14
    ip, _, mp, _ = lc.write_set(tmp_path, n)
    loader = tl.TileLoader({"IMG": ip, "MSK": mp}, _feed("without"), batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(5),
                           device=dev, cache_bytes=9 * ITEM)
    replay = torch.Generator().manual_seed(5)
    for epoch in range(3):
        order = tl.epoch_batches(n, 4, True, False, replay)
        batches = list(loader)
        torch.cuda.synchronize()
        assert [b["img"].shape[0] for b in batches] == [4, 4, 4, 2]
        assert len({b["img"].data_ptr() for b in batches}) == 4 and len({b["msk"].data_ptr() for b in batches}) == 4
        slabs = (loader.cache.img, loader.cache.msk)
        for b, idx in zip(batches, order, strict=True):
            _assert_batch(b, idx, n, "without")
            for t in (b["img"], b["msk"]):          # a batch owns its tensors: none of them is a view of a slab
                assert all(t.untyped_storage().data_ptr() != s.untyped_storage().data_ptr() for s in slabs)
    assert loader.cache_stats["resident"] == 9


def test_predict_split_and_metadata_with_a_cache(dev, tmp_path):
    n = 5
    ip, img, mp, _ = lc.write_set(tmp_path, n)
    mtd = np.random.default_rng(4).random((n, 45))
    config = {"batch_size": 4, "channels": [1, 2, 3, 4, 5], "classes": {i + 1: [1, str(i)] for i in range(13)}, "norm_type": "without",
              "norm_means": [], "norm_stds": [], "use_augmentation": True, "use_metadata": True}
    loader = tl.TileLoader.from_config(config, {"IMG": ip, "MSK": mp, "MTD": mtd.tolist()}, "predict", device=dev, cache_bytes=3 * 32 * 32 * 5)
    for epoch in range(2):
        pred = list(loader)
        assert len(pred) == n
        for s, b in enumerate(pred):
            assert sorted(b) == ["id", "img", "mtd"] and b["id"] == [ip[s]]
            assert np.array_equal(b["img"][0].cpu().numpy(), img[s].astype(np.float32))
            assert torch.equal(b["mtd"].cpu(), torch.as_tensor(mtd[s:s + 1], dtype=torch.float32))
    assert loader.cache.msk is None and tuple(loader.cache.img.shape) == (3, 5, 32, 32)      # an item is its image alone
    assert loader.cache_stats == {"hits": 3, "misses": 2 * n - 3, "files_read": 2 * n - 3, "resident": 3, "capacity": 3}
