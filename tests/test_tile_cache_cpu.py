"""CPU suite of the tile cache's bookkeeping (flair_amd/tile_cache.py: SlotBook, the host half of TileCache) and of how TileLoader
takes ``cache_bytes``: pure host code, no device call.  Integer work: every assertion is exact."""
import numpy as np
import pytest

from flair_amd import tile_cache as tc
from flair_amd import tile_loader as tl

ITEM = 32 * 32 * 6   # a 32 x 32 tile of five bands and its mask


def _book(n_items=12, slots=5):
    book = tc.SlotBook(n_items, slots * ITEM + ITEM - 1)      # the odd bytes buy no further slot
    assert not book.is_open and book.stats == {"hits": 0, "misses": 0, "files_read": 0, "resident": 0, "capacity": 0}
    assert book.open(ITEM) == slots and book.is_open
    return book


def test_capacity_is_the_budget_in_items_and_at_most_every_item():
    assert tc.SlotBook(12, 5 * ITEM).open(ITEM) == 5
    assert tc.SlotBook(12, 5 * ITEM - 1).open(ITEM) == 4
    assert tc.SlotBook(12, 100 * ITEM).open(ITEM) == 12
    assert tc.SlotBook(12, ITEM - 1).open(ITEM) == 0
    assert tc.SlotBook(0, 5 * ITEM).open(ITEM) == 0
    book = tc.SlotBook(12, ITEM - 1)
    book.open(ITEM)
    assert book.assign([0, 1]) == [-1, -1] and book.stats["capacity"] == 0      # nothing to give: the loader's plain path
    with pytest.raises(RuntimeError):
        book.open(ITEM)
    with pytest.raises(ValueError):
        tc.SlotBook(12, 5 * ITEM).open(0)
    with pytest.raises(ValueError):
        tc.SlotBook(12, -1)


def test_assign_up_to_capacity_then_none():
    book = _book()
    assert book.assign([7, 3, 9]) == [0, 1, 2] and book.free_slots == 2
    assert book.assign([4, 5, 6, 8]) == [3, 4, -1, -1] and book.free_slots == 0
    assert book.assign([10]) == [-1]
    assert book.resident == 0 and (book.slot_of == -1).all()          # assigned is not resident
    with pytest.raises(RuntimeError):
        book.assign([7])                                              # pending already


def test_commit_makes_resident_and_release_gives_back():
    book = _book()
    book.assign([7, 3, 9])
    book.commit([7, 9])
    assert book.resident == 2 and book.slot_of[7] == 0 and book.slot_of[9] == 2 and book.slot_of[3] == -1
    book.release([3])
    assert book.free_slots == 3 and book.resident == 2
    book.release([7])                                                 # resident, not pending: nothing happens
    assert book.free_slots == 3 and book.slot_of[7] == 0
    assert sorted(book.assign([1, 2, 4, 5])) == [-1, 1, 3, 4]         # the slot given back is given out again
    book.commit([6])                                                  # never assigned: nothing happens
    assert book.slot_of[6] == -1
    with pytest.raises(RuntimeError):
        book.assign([9])                                              # resident already
    assert book.lookup([7, 3, 9, 1]).tolist() == [0, -1, 2, -1]       # 1 is pending, not resident


def test_an_abandoned_jobs_slots_return():
    book = _book()
    book.assign([0, 1])
    book.commit([0, 1])
    book.assign([2, 3])                     # a job that is never finished
    book.assign([4, 5])                     # and the one behind it: one slot left
    assert book.free_slots == 0
    book.abandon()
    assert book.free_slots == 3 and book.resident == 2
    assert sorted(book.assign([2, 3, 4, 5])) == [-1, 2, 3, 4]
    book.commit([2, 3, 4, 5])
    assert book.resident == 5 and book.free_slots == 0
    assert sorted(book.slot_of[book.slot_of >= 0].tolist()) == [0, 1, 2, 3, 4]   # no slot lost, none given twice


def test_clear_forgets_every_item():
    book = _book()
    book.lookup([0, 1, 2])
    book.assign([0, 1, 2])
    book.commit([0, 1])
    book.files_read += 6
    book.clear()
    assert book.stats == {"hits": 0, "misses": 0, "files_read": 0, "resident": 0, "capacity": 5}
    assert book.free_slots == 5 and book.lookup([0, 1, 2]).tolist() == [-1, -1, -1]
    book.commit([2])                                                  # what was pending before clear() is forgotten too
    assert book.resident == 0
    assert book.assign([8, 9, 10, 11, 0, 1]) == [0, 1, 2, 3, 4, -1]


def test_statistics_add_up():
    book = _book()
    rng = np.random.default_rng(0)
    asked = 0
    for epoch in range(3):
        order = rng.permutation(12).tolist()
        for at in range(0, 12, 4):
            idx = order[at:at + 4]
            slots = book.lookup(idx)
            absent = [i for i, s in zip(idx, slots) if s < 0]
            book.files_read += 2 * len(absent)
            book.assign(absent)
            book.commit(absent)
            asked += len(idx)
            s = book.stats
            assert s["hits"] + s["misses"] == asked and s["files_read"] == 2 * s["misses"] and s["resident"] <= s["capacity"] == 5
    s = book.stats
    assert s["resident"] == 5 and s["misses"] == 12 + 2 * 7 and s["hits"] == 2 * 5      # five items hit in each later epoch


def test_cache_bytes_zero_constructs_no_cache(tmp_path):
    files = {"IMG": [str(tmp_path / f"IMG_{i}.tif") for i in range(12)], "MSK": [str(tmp_path / f"MSK_{i}.tif") for i in range(12)]}
    feed = lambda i, m, mtd=None, ids=None: {"img": i, "msk": m}   # noqa: E731
    plain = tl.TileLoader(files, feed, batch_size=4)
    assert plain.cache is None and plain.cache_stats is None
    assert tl.TileLoader(files, feed, batch_size=4, cache_bytes=0).cache is None
    with pytest.raises(TypeError, match="from_sources"):
        tl.TileLoader(files, feed, batch_size=4, cache_bytes=1 << 20)       # a cache feeds through TileFeed.from_sources
    with pytest.raises(ValueError):
        tl.TileLoader(files, feed, batch_size=4, cache_bytes=-1)
    from flair_amd.data_feed import TileFeed
    cached = tl.TileLoader(files, TileFeed([1, 2, 3, 4, 5], 13, "scaling"), batch_size=4, cache_bytes=5 * ITEM)
    assert isinstance(cached.cache, tc.TileCache) and cached.cache.n_items == 12 and not cached.cache.is_open   # no slab before a batch
    assert cached.cache_stats == {"hits": 0, "misses": 0, "files_read": 0, "resident": 0, "capacity": 0}
    assert cached.cache.img is None and cached.cache.msk is None


def test_from_config_takes_the_argument_and_the_environment(tmp_path, monkeypatch):
    config = {"batch_size": 4, "channels": [1, 2, 3, 4, 5], "classes": {i + 1: [1, str(i)] for i in range(13)}, "norm_type": "scaling",
              "norm_means": [], "norm_stds": [], "use_augmentation": False, "use_metadata": False}
    files = {"IMG": [str(tmp_path / f"IMG_{i}.tif") for i in range(12)], "MSK": [str(tmp_path / f"MSK_{i}.tif") for i in range(12)]}
    monkeypatch.delenv("FLAIR_TILE_CACHE_GB", raising=False)
    assert tl.TileLoader.from_config(config, files, "train").cache is None
    assert tl.TileLoader.from_config(config, files, "val", cache_bytes=3 * ITEM).cache.cache_bytes == 3 * ITEM
    monkeypatch.setenv("FLAIR_TILE_CACHE_GB", "1.5")
    assert tl.TileLoader.from_config(config, files, "train").cache.cache_bytes == 1_500_000_000
    assert tl.TileLoader.from_config(config, files, "train", cache_bytes=0).cache is None       # the argument goes before the environment
    assert tl.TileLoader.from_config(config, files, "predict", cache_bytes=ITEM).cache.cache_bytes == ITEM
