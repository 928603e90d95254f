"""Decoded tiles kept in HBM between epochs (DESIGN.md §10 "Tile cache").  ``TileLoader`` decodes the IMG / MSK files of every batch
on the device; every epoch after the first decodes the same bytes again.  With a cache the decoded uint8 tiles of an item stay in a
slot of a slab, and a later batch is one launch of ``flair_feed_tiles_ptrs`` over the slots' addresses.

``SlotBook`` is the bookkeeping: which item holds which slot, pure host code with no torch device call.  ``TileCache`` adds the two
slabs.  There is no eviction: items get slots in the order they are first seen until the slots are used up, later items are decoded
every time.  The cache is keyed by the item's index in the loader's file list and never looks at a file again once the item is
resident; ``clear()`` is the caller's remedy when files change on disk.
"""
from __future__ import annotations

import numpy as np
import torch


class SlotBook:
    """``slot_of[item]`` (-1: absent) over ``n_items`` items and a budget of ``cache_bytes``.  The capacity follows from the bytes
    of one item, known at the first batch (``open``).  A slot is assigned when a job begins (``assign``) and the item becomes
    resident only when its batch has finished cleanly (``commit``); ``release`` gives the slots of a job that raised back, ``abandon``
    those of every job that was never finished."""

    def __init__(self, n_items: int, cache_bytes: int):
        self.n_items, self.cache_bytes = int(n_items), int(cache_bytes)
        if self.n_items < 0 or self.cache_bytes < 0:
            raise ValueError(f"n_items and cache_bytes must not be negative, got {n_items} and {cache_bytes}")
        self.slot_of = np.full(self.n_items, -1, dtype=np.int64)
        self.item_bytes = None
        self.capacity = None          # slots; None until open()
        self._free = []
        self._pending = {}            # item -> slot, assigned and not yet committed
        self.hits = self.misses = self.files_read = 0

    @property
    def is_open(self) -> bool:
        return self.capacity is not None

    def open(self, item_bytes: int) -> int:
        """fixes the capacity, ``min(n_items, cache_bytes // item_bytes)`` slots, and returns it"""
        if self.is_open:
            raise RuntimeError("the slot book is open already")
        if item_bytes < 1:
            raise ValueError(f"item_bytes must be positive, got {item_bytes}")
        self.item_bytes = int(item_bytes)
        self.capacity = min(self.n_items, self.cache_bytes // self.item_bytes)
        self._free = list(range(self.capacity - 1, -1, -1))   # popped from the end: slot 0 first
        return self.capacity

    @property
    def resident(self) -> int:
        return int((self.slot_of >= 0).sum())

    @property
    def free_slots(self) -> int:
        return len(self._free)

    def lookup(self, items) -> np.ndarray:
        """the slots of ``items``, -1 for the absent ones; counts one hit or one miss per item"""
        slots = self.slot_of[np.asarray(items, dtype=np.int64)]
        hits = int((slots >= 0).sum())
        self.hits += hits
        self.misses += len(slots) - hits
        return slots

    def assign(self, items) -> list:
        """a free slot (or -1 when none is left) for each of ``items``, none of which is resident or pending"""
        out = []
        for item in items:
            item = int(item)
            if self.slot_of[item] >= 0 or item in self._pending:
                raise RuntimeError(f"item {item} holds a slot already")
            slot = self._free.pop() if self._free else -1
            if slot >= 0:
                self._pending[item] = slot
            out.append(slot)
        return out

    def commit(self, items) -> None:
        """the pending ones of ``items`` are resident from now on"""
        for item in items:
            slot = self._pending.pop(int(item), -1)
            if slot >= 0:
                self.slot_of[int(item)] = slot

    def release(self, items) -> None:
        """the pending ones of ``items`` give their slots back and stay absent"""
        for item in items:
            slot = self._pending.pop(int(item), -1)
            if slot >= 0:
                self._free.append(slot)

    def abandon(self) -> None:
        """every pending assignment is released: jobs that were begun and never finished"""
        self.release(list(self._pending))

    def clear(self) -> None:
        """forgets every item, resident or pending, and starts the statistics again; the capacity stays"""
        self.slot_of[:] = -1
        self._pending.clear()
        if self.is_open:
            self._free = list(range(self.capacity - 1, -1, -1))
        self.hits = self.misses = self.files_read = 0

    @property
    def stats(self) -> dict:
        return {"hits": self.hits, "misses": self.misses, "files_read": self.files_read, "resident": self.resident,
                "capacity": 0 if self.capacity is None else self.capacity}


class TileCache(SlotBook):
    """``SlotBook`` plus the slabs on ``device``: ``img`` (capacity, bands, H, W) uint8 and, where the loader has masks, ``msk``
    (capacity, H, W) uint8, allocated by ``allocate`` at the first batch, when the shape is known.  An item is ``bands * H * W`` bytes
    plus ``H * W`` with masks.

    Stream rule: the slabs are written (``store``) and read (the feed launch over ``addresses``) only on the stream that is current
    when ``TileLoader._finish`` runs, so the writes of a slot and every later read of it are in stream order.  A caller that iterates
    under changing streams must synchronise them itself."""

    def __init__(self, n_items: int, cache_bytes: int, device):
        super().__init__(n_items, cache_bytes)
        self.device = torch.device(device)
        self.shape = None             # (bands, H, W)
        self.img = self.msk = None

    def allocate(self, bands: int, H: int, W: int, masks: bool) -> None:
        self.shape = (int(bands), int(H), int(W))
        cap = self.open(bands * H * W + (H * W if masks else 0))
        if cap:
            self.img = torch.empty(cap, bands, H, W, dtype=torch.uint8, device=self.device)
            self.msk = torch.empty(cap, H, W, dtype=torch.uint8, device=self.device) if masks else None

    def store(self, slots: torch.Tensor, img_u8: torch.Tensor, msk_raw: torch.Tensor | None) -> None:
        """one indexed copy per kind on the current stream: row i of ``img_u8`` / ``msk_raw`` into slot ``slots[i]``"""
        self.img.index_copy_(0, slots, img_u8)
        if self.msk is not None:
            self.msk.index_copy_(0, slots, msk_raw)

    def addresses(self, slots: np.ndarray):
        """(image addresses, mask addresses or None) of ``slots`` as int64 arrays"""
        bands, H, W = self.shape
        img = self.img.data_ptr() + slots * (bands * H * W)
        return img, (None if self.msk is None else self.msk.data_ptr() + slots * (H * W))
