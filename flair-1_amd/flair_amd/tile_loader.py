"""From the dataset on disk to the step's batch (the disk half): the reference's ``fit_dataset`` / ``predict_dataset``
behind a ``DataLoader`` (src/flair/data_loader.py:34-144, data_module.py:79-104) read one tile per rasterio call on CPU workers.
Here the IMG and MSK files of a whole batch are read into one pinned buffer, go up in one copy per kind, are decoded by one launch
of ``ops.tiff_lzw_decode_chunks`` per kind (stored and LZW chunks, tiles and strips, one wave per chunk) and scattered by one launch
of ``ops.tiff_chunks_to_batch`` (csrc/tiff_read.hip) into the ``(B, bands, H, W)`` and ``(B, H, W)`` uint8 tensors ``TileFeed`` takes.
Only the files' bytes cross PCIe.  ``TileLoader`` begins batch n + 1 before it hands out batch n, so the host's file reads and the
upload run under the caller's step.  With ``cache_bytes`` the decoded tiles stay in HBM (``tile_cache.py``) and later epochs are fed
from there.

The files are those ``raster_reader.raster_layout`` accepts, and they may differ in layout inside a batch.  There is no fallback
reader: a file outside the family is refused by name (``UnsupportedRaster``) before any device work.
"""
from __future__ import annotations

import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass

import numpy as np
import torch

from .raster_reader import FLUSH_BLOCK, RasterLayout, UnsupportedRaster, raise_if_failed, raster_layout
from .tiff_staging import GROUP_BYTES, PinnedPair, stream_groups
from .tile_cache import TileCache

READ_THREADS = 16   # file reads of a batch in flight; a fixed number, whatever the machine's CPU count


def _align16(n):
    return (n + 15) & ~15


@dataclass
class BatchPlan:
    """One decode launch and one scatter launch over the chunks of a batch of files of one kind.  The files lie one behind the other
    in the source buffer, file i at ``bases[i]`` (multiples of 16); chunk j of the batch is chunk ``j - first[owner[j]]`` of file
    ``owner[j]``.  ``table``: (n, 8) int32 rows {x0, y0, width, rows, plane0, samples, predictor, 0} as flair_tiff_chunks_to_batch
    takes them, plane0 = file * bands + band0.  ``groups``: (first, n) chunk windows whose slots fit ``group_bytes``."""
    layouts: list
    H: int
    W: int
    bands: int
    bases: np.ndarray
    src_bytes: int
    slot: int
    groups: list
    src_off: np.ndarray     # int64
    src_len: np.ndarray     # int32, as dst_len and mode
    dst_len: np.ndarray
    mode: np.ndarray
    table: np.ndarray
    owner: np.ndarray
    first: np.ndarray
    max_rows: int

    @property
    def n_chunks(self) -> int:
        return len(self.owner)


def _label(names, i):
    return f"file {i}" if names is None else repr(os.fspath(names[i]))


def plan_batch(files, group_bytes: int = GROUP_BYTES, names=None, shape=None) -> BatchPlan:
    """The plan of one kind of file of a batch.  ``files``: the bytes (bytes, memoryview, mmap) of every whole file; ``names``: their
    paths, for the messages.  Every file goes through ``raster_layout``; a file outside its family raises ``UnsupportedRaster``
    naming the file, a file whose (bands, H, W) is not ``shape`` (default: the first file's) raises ``ValueError`` naming it.  The
    slot is uniform: the largest chunk of the batch rounded up to the decoder's flush block."""
    if not len(files):
        raise ValueError("plan_batch needs at least one file")
    layouts = []
    for i, data in enumerate(files):
        try:
            if len(data) < 8:
                raise UnsupportedRaster("not a TIFF: fewer than 8 bytes")
            layouts.append(raster_layout(data))
        except UnsupportedRaster as err:
            raise UnsupportedRaster(f"{_label(names, i)}: {err}") from None
    first: RasterLayout = layouts[0]
    want = tuple(shape) if shape is not None else (first.bands, first.H, first.W)
    for i, lay in enumerate(layouts):
        if (lay.bands, lay.H, lay.W) != want:
            raise ValueError(f"{_label(names, i)} is {lay.bands} x {lay.H} x {lay.W} (bands x H x W), not {want[0]} x {want[1]} x {want[2]} "
                             f"like {'the batch' if shape is not None else _label(names, 0)}: the files of a batch share one shape")
    bands, H, W = want
    bases = np.zeros(len(files), dtype=np.int64)
    at = 0
    for i, data in enumerate(files):
        bases[i] = at
        at += _align16(len(data))
    src_off, src_len, dst_len, mode, tables, owner = [], [], [], [], [], []
    for i, lay in enumerate(layouts):
        t5, sl, dl, md = lay.decode_tables()
        t8 = np.zeros((lay.n_chunks, 8), dtype=np.int32)
        t8[:, :4] = t5[:, :4]
        t8[:, 4] = i * lay.bands + t5[:, 4]
        t8[:, 5], t8[:, 6] = lay.samples, lay.predictor
        src_off.append(bases[i] + lay.offsets)
        src_len.append(sl), dst_len.append(dl), mode.append(md), tables.append(t8)
        owner.append(np.full(lay.n_chunks, i, dtype=np.int64))
    counts = np.array([lay.n_chunks for lay in layouts], dtype=np.int64)
    table = np.concatenate(tables)
    slot = max(lay.slot_bytes for lay in layouts)
    assert slot % FLUSH_BLOCK == 0
    groups = stream_groups(len(table), 1, slot, group_bytes)
    return BatchPlan(layouts, H, W, bands, bases, at, slot, groups, np.concatenate(src_off).astype(np.int64),
                     np.concatenate(src_len), np.concatenate(dst_len), np.concatenate(mode), table, np.concatenate(owner),
                     np.cumsum(counts) - counts, int(table[:, 3].max()))


def plan_tiles(img_files, msk_files=None, group_bytes: int = GROUP_BYTES, img_names=None, msk_names=None):
    """(image plan, mask plan or None) of a batch: ``plan_batch`` of either kind, the masks held to the images: as many files, each a
    single band of the images' H x W, else ``ValueError`` naming the mask.  Pure host work."""
    img = plan_batch(img_files, group_bytes, img_names)
    if msk_files is None:
        return img, None
    if len(msk_files) != len(img_files):
        raise ValueError(f"{len(msk_files)} masks for {len(img_files)} images")
    return img, plan_batch(msk_files, group_bytes, msk_names, shape=(1, img.H, img.W))


# ------------------------------------------------------------------------------------------------------------------ the device half
_pool = None
_staging = PinnedPair()   # the file bytes of a batch; taken in turn: batch n's copy may be in flight while batch n + 1 is read
_copy_streams = {}


def _read_pool():
    global _pool
    if _pool is None:
        _pool = ThreadPoolExecutor(max_workers=READ_THREADS, thread_name_prefix="flair-tile-read")
    return _pool


def _copy_stream(dev):
    if dev not in _copy_streams:
        _copy_streams[dev] = torch.cuda.Stream(device=dev)
    return _copy_streams[dev]


def _read_into(args):
    path, view = args
    with open(path, "rb") as f:
        got = f.readinto(view)
        if got != len(view) or f.read(1):
            raise OSError(f"{path!r} changed size while it was read: {got} of {len(view)} bytes")


class PendingTiles:
    """what begin_read_tiles leaves for finish_read_tiles: decode and scatter are queued, the status not yet read"""

    def __init__(self, img_paths, msk_paths):
        self.img_paths, self.msk_paths = img_paths, msk_paths
        self.kinds = []        # (paths, plan, planes, pinned status) per kind
        self.done = None       # the event behind the last status copy
        self.keep = []         # the device buffers the queued work reads


def _tables_pinned(plan: BatchPlan):
    """[src_off int64 | src_len | dst_len | mode | table] of a plan in one pinned byte tensor, and where each begins"""
    n = plan.n_chunks
    t = torch.empty(8 * n + 4 * (3 * n + 8 * n), dtype=torch.uint8, pin_memory=True)
    a = t.numpy()
    a[:8 * n].view(np.int64)[:] = plan.src_off
    a[8 * n:].view(np.int32)[:] = np.concatenate([plan.src_len, plan.dst_len, plan.mode, plan.table.reshape(-1)])
    return t


def begin_read_tiles(img_paths, msk_paths=None, device="cuda", group_bytes: int = GROUP_BYTES) -> PendingTiles:
    """The first half of read_tiles, without a wait for the device: reads the files of both kinds into one pinned buffer (a pool of
    ``READ_THREADS`` threads), plans the batch (``plan_tiles``: refusals are raised here, before any device work), and on a side
    stream uploads the bytes in one copy per kind, queues decode and scatter and, behind them, the copy of the status to pinned
    memory.  The caller's stream is not involved until ``finish_read_tiles`` has waited for that copy."""
    from . import ops
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("read_tiles decodes on the HIP device")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    img_paths = [os.fspath(p) for p in img_paths]
    msk_paths = None if msk_paths is None else [os.fspath(p) for p in msk_paths]
    paths = img_paths + (msk_paths or [])
    sizes = [os.stat(p).st_size for p in paths]
    bases, total = [], 0
    for s in sizes:
        bases.append(total)
        total += _align16(s)
    with torch.cuda.device(dev):
        staging, turn = _staging.take_next(max(total, 16))
        raw = staging.numpy()
        views = [memoryview(raw[b:b + s]) for b, s in zip(bases, sizes)]
        list(_read_pool().map(_read_into, [(p, v) for p, v in zip(paths, views) if len(v)]))
        n_img = len(img_paths)
        img_plan, msk_plan = plan_tiles(views[:n_img], None if msk_paths is None else views[n_img:], group_bytes, img_paths, msk_paths)
        job = PendingTiles(img_paths, msk_paths)
        kinds = [(img_paths, img_plan, bases[0], (n_img, img_plan.bands))]
        if msk_plan is not None:
            kinds.append((msk_paths, msk_plan, bases[n_img], (n_img,)))
        # Everything runs on the side stream, whose buffers are its own: nothing here waits for the caller's stream or makes it wait,
        # so the decode of batch n + 1, a few hundred serial waves, runs beside the step of batch n and not in front of it.
        with torch.cuda.stream(_copy_stream(dev)):
            uploads = []
            for _, plan, base, _ in kinds:   # the copies first: the second kind's bytes go up under the first kind's decode
                d_src = torch.empty(max(plan.src_bytes, 16), dtype=torch.uint8, device=dev)
                d_src[:plan.src_bytes].copy_(staging[base:base + plan.src_bytes], non_blocking=True)
                uploads.append((d_src, _tables_pinned(plan).to(dev, non_blocking=True)))
            _staging.copied(turn)
            for (paths_k, plan, _, lead), (d_src, d_tab) in zip(kinds, uploads):
                n = plan.n_chunks
                src_off = d_tab[:8 * n].view(torch.int64)
                i32 = d_tab[8 * n:].view(torch.int32)
                src_len, dst_len, mode, table = i32[:n], i32[n:2 * n], i32[2 * n:3 * n], i32[3 * n:].view(n, 8)
                planes = torch.empty(*lead, plan.H, plan.W, dtype=torch.uint8, device=dev)
                status = torch.empty(n, dtype=torch.int32, device=dev)
                scratch = torch.empty(max(k for _, k in plan.groups) * plan.slot, dtype=torch.uint8, device=dev)
                for first, k in plan.groups:   # one launch each where the slots fit group_bytes; the scratch is reused in stream order
                    sl = slice(first, first + k)
                    slots, st = ops.tiff_lzw_decode_chunks(d_src, src_off[sl], src_len[sl], dst_len[sl], mode[sl], plan.slot,
                                                           out=scratch[:k * plan.slot], status=status[sl])
                    ops.tiff_chunks_to_batch(slots, table[sl], st, planes, max_rows=plan.max_rows)
                status_h = torch.empty(n, dtype=torch.int32, pin_memory=True)
                status_h.copy_(status, non_blocking=True)
                job.kinds.append((paths_k, plan, planes, status_h))
                job.keep += [d_src, d_tab, status, scratch]
            job.done = torch.cuda.Event()
            job.done.record()
    return job


def finish_read_tiles(job: PendingTiles):
    """The second half: waits for the batch's status and returns (img_u8 (B, bands, H, W), msk_raw (B, H, W) or None), both uint8 on
    the device and owned by the caller.  A chunk whose status is not 0 raises ``RasterDecodeError`` naming its file and the chunk."""
    job.done.synchronize()
    job.keep.clear()
    out = []
    for paths, plan, planes, status_h in job.kinds:
        status = status_h.numpy()
        if status.any():
            i = int(plan.owner[np.flatnonzero(status)[0]])
            lay = plan.layouts[i]
            raise_if_failed(paths[i], lay, status[plan.first[i]:plan.first[i] + lay.n_chunks])
        planes.record_stream(torch.cuda.current_stream(planes.device))   # made on the side stream, used and freed on the caller's
        out.append(planes)
    return out[0], (out[1] if len(out) > 1 else None)


def read_tiles(img_paths, msk_paths=None, device="cuda", group_bytes: int = GROUP_BYTES):
    """(img_u8 (B, bands, H, W), msk_raw (B, H, W) or None) of a batch of tile files, decoded on the device"""
    return finish_read_tiles(begin_read_tiles(img_paths, msk_paths, device, group_bytes))


# ------------------------------------------------------------------------------------------------------------------------ the loader
def epoch_batches(n: int, batch_size: int, shuffle: bool, drop_last: bool, generator: torch.Generator | None = None) -> list:
    """The index lists of one epoch over n files, as a DataLoader's sampler and batch sampler make them: a permutation drawn from
    ``generator`` when ``shuffle``, file order otherwise, cut into batches of ``batch_size``, the short last one dropped or kept."""
    n, batch_size = int(n), int(batch_size)
    if batch_size < 1:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    order = torch.randperm(n, generator=generator).tolist() if shuffle else list(range(n))
    batches = [order[i:i + batch_size] for i in range(0, n, batch_size)]
    if drop_last and batches and len(batches[-1]) < batch_size:
        batches.pop()
    return batches


class TileLoader:
    """``flair_datamodule``'s DataLoaders over ``dict_files`` = {'IMG': paths, 'MSK': paths (fit), 'MTD': 45-vectors (metadata)}, as
    ``gather_paths`` makes it: iterating yields the batch dicts of ``fit_dataset`` (``img`` fp32 NCHW, ``msk`` as class indices,
    ``mtd``) or, without 'MSK', of ``predict_dataset`` (``img``, ``mtd``, ``id`` the image paths), made by ``feed`` (a ``TileFeed``)
    from the files' bytes on ``device``.  Batch n + 1 is begun (read, uploaded, decode queued) before batch n is yielded; every
    yielded batch owns its tensors.

    ``cache_bytes`` > 0 keeps the decoded uint8 tiles in HBM (``tile_cache.TileCache``, at most that many bytes; ``feed`` must then
    have ``TileFeed.from_sources``): an item is read and decoded the first time it is asked for, copied into a slot when its batch
    has finished cleanly, and fed from the slot ever after, without a look at its files; items that find no free slot are decoded
    every time.  ``cache_stats`` counts it, ``cache.clear()`` (between epochs) forgets every item.  A slot is assigned when a job
    begins and committed when its batch is yielded; the slots of a batch that raised, or that was begun and never yielded because
    the caller left the loop, are free again, and one iteration over a loader at a time is all a cache supports.  Stream rule: the
    slabs are written and read only on the stream that is current when a batch is finished (inside ``next()``), so the writes of
    a slot and all later reads of it are in stream order; a caller that iterates under changing streams must synchronise them
    itself."""

    def __init__(self, dict_files: dict, feed, batch_size: int = 2, shuffle: bool = False, drop_last: bool = False,
                 generator: torch.Generator | None = None, device="cuda", use_metadata: bool | None = None,
                 group_bytes: int = GROUP_BYTES, cache_bytes: int = 0):
        self.imgs = [os.fspath(p) for p in dict_files["IMG"]]
        self.msks = [os.fspath(p) for p in dict_files["MSK"]] if dict_files.get("MSK") is not None and len(dict_files["MSK"]) else None
        if self.msks is not None and len(self.msks) != len(self.imgs):
            raise ValueError(f"{len(self.msks)} masks for {len(self.imgs)} images")
        if use_metadata is None:
            use_metadata = dict_files.get("MTD") is not None and len(dict_files["MTD"]) > 0
        self.mtd = None
        if use_metadata:
            self.mtd = torch.as_tensor(np.asarray(dict_files["MTD"], dtype=np.float64), dtype=torch.float32)
            if self.mtd.dim() != 2 or self.mtd.shape[0] != len(self.imgs):
                raise ValueError(f"'MTD' must hold one vector per image, got {tuple(self.mtd.shape)} for {len(self.imgs)} images")
        self.feed, self.batch_size, self.shuffle, self.drop_last = feed, int(batch_size), bool(shuffle), bool(drop_last)
        self.generator, self.device, self.group_bytes = generator, torch.device(device), group_bytes
        self.cache = None
        if int(cache_bytes) < 0:
            raise ValueError(f"cache_bytes must not be negative, got {cache_bytes}")
        if int(cache_bytes) > 0:
            if not hasattr(feed, "from_sources"):
                raise TypeError("a tile cache feeds batches through feed.from_sources (TileFeed), which this feed does not have")
            self.cache = TileCache(len(self.imgs), int(cache_bytes), self.device)

    @classmethod
    def from_config(cls, config: dict, dict_files: dict, split: str, device="cuda", generator=None,
                    cache_bytes: int | None = None) -> "TileLoader":
        """The loader of ``split`` ('train' | 'val' | 'predict') as data_module.py:79-104 and tasks_utils.get_data_module set it:
        config['batch_size'] shuffled (train) or in file order (val), both with drop_last=True; predict: one tile a batch, in file
        order, nothing dropped.  ``cache_bytes`` as in the constructor; not given, it is the environment's ``FLAIR_TILE_CACHE_GB``
        (gigabytes of 10^9 bytes, fractions allowed) or 0."""
        from .data_feed import TileFeed
        if split not in ("train", "val", "predict"):
            raise ValueError(f"split must be 'train', 'val' or 'predict', got {split!r}")
        if cache_bytes is None:
            cache_bytes = int(float(os.environ.get("FLAIR_TILE_CACHE_GB") or 0) * 1e9)
        feed = TileFeed.from_config(config, train=split == "train", generator=generator)
        fit = split != "predict"
        files = dict_files if fit else {k: v for k, v in dict_files.items() if k != "MSK"}
        return cls(files, feed, batch_size=config["batch_size"] if fit else 1, shuffle=split == "train", drop_last=fit,
                   generator=generator, device=device, use_metadata=bool(config.get("use_metadata", False)), cache_bytes=cache_bytes)

    @property
    def cache_stats(self):
        """{'hits', 'misses', 'files_read', 'resident', 'capacity'} counted per item (``files_read`` per file) since construction or
        ``cache.clear()``; None without a cache"""
        return None if self.cache is None else self.cache.stats

    def __len__(self) -> int:
        n = len(self.imgs)
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def _begin(self, idx):
        if self.cache is not None:
            return self._begin_cached(idx)
        job = begin_read_tiles([self.imgs[i] for i in idx], None if self.msks is None else [self.msks[i] for i in idx], self.device,
                               self.group_bytes)
        return idx, job

    def _finish(self, pending) -> dict:
        if self.cache is not None:
            return self._finish_cached(pending)
        idx, job = pending
        img_u8, msk_raw = finish_read_tiles(job)
        with torch.cuda.device(self.device):
            return self.feed(img_u8, msk_raw, mtd=None if self.mtd is None else self.mtd[idx],
                             ids=[self.imgs[i] for i in idx] if self.msks is None else None)

    def _begin_cached(self, idx):
        """(idx, slots of the resident items (-1: absent), positions of the absent ones, the slots those were assigned (-1: none left),
        their job or None): only the absent items are read and decoded, and a batch without one queues nothing"""
        cache = self.cache
        slots = cache.lookup(idx)
        absent = np.flatnonzero(slots < 0)
        if not len(absent):
            return idx, slots, absent, np.empty(0, dtype=np.int64), None
        items = [idx[p] for p in absent]
        job = begin_read_tiles([self.imgs[i] for i in items], None if self.msks is None else [self.msks[i] for i in items], self.device,
                               self.group_bytes)
        cache.files_read += len(items) * (1 if self.msks is None else 2)
        plan = job.kinds[0][1]
        if not cache.is_open:    # the first batch: the shape of an item, and with it the capacity, is known now
            with torch.cuda.device(self.device):
                cache.allocate(plan.bands, plan.H, plan.W, self.msks is not None)
        elif (plan.bands, plan.H, plan.W) != cache.shape:
            raise ValueError(f"{_label(self.imgs, items[0])} is {plan.bands} x {plan.H} x {plan.W} (bands x H x W), not "
                             f"{cache.shape[0]} x {cache.shape[1]} x {cache.shape[2]} like the cached tiles: a cache holds one shape")
        return idx, slots, absent, np.asarray(cache.assign(items), dtype=np.int64), job

    def _finish_cached(self, pending) -> dict:
        idx, slots, absent, assigned, job = pending
        cache = self.cache
        items = [idx[p] for p in absent]
        mtd = None if self.mtd is None else self.mtd[idx]
        ids = [self.imgs[i] for i in idx] if self.msks is None else None
        try:
            img_u8 = msk_raw = None
            if job is not None:
                img_u8, msk_raw = finish_read_tiles(job)    # a failed chunk raises here: nothing of the batch has reached a slab
            with torch.cuda.device(self.device):
                if len(absent) == len(idx) and not (assigned >= 0).any():   # nothing of the batch is or becomes resident: as without a cache
                    return self.feed(img_u8, msk_raw, mtd=mtd, ids=ids)
                B, (bands, H, W) = len(idx), cache.shape
                kept = np.flatnonzero(assigned >= 0)       # the rows of the job's tensors that go into a slot
                slots = slots.copy()
                slots[absent] = assigned
                in_slab = slots >= 0
                # [image addresses (B) | mask addresses (B) | slots of the kept rows | the kept rows], up from pinned memory in one copy
                table = torch.empty(2 * B + 2 * len(kept), dtype=torch.int64, pin_memory=True)
                t = table.numpy()
                t[:2 * B] = 0
                img_at, msk_at = cache.addresses(slots[in_slab])
                t[:B][in_slab] = img_at
                if msk_at is not None:
                    t[B:2 * B][in_slab] = msk_at
                loose = assigned < 0                        # decoded and without a slot: fed from the job's own tensors
                if loose.any():
                    rows = np.flatnonzero(loose)
                    t[:B][absent[loose]] = img_u8.data_ptr() + rows * (bands * H * W)
                    if msk_raw is not None:
                        t[B:2 * B][absent[loose]] = msk_raw.data_ptr() + rows * (H * W)
                t[2 * B:2 * B + len(kept)] = assigned[kept]
                t[2 * B + len(kept):] = kept
                d = table.to(self.device, non_blocking=True)
                if len(kept):
                    whole = len(kept) == len(absent)
                    rows_d = d[2 * B + len(kept):]
                    cache.store(d[2 * B:2 * B + len(kept)], img_u8 if whole else img_u8.index_select(0, rows_d),
                                msk_raw if whole or msk_raw is None else msk_raw.index_select(0, rows_d))
                batch = self.feed.from_sources(d[:B], None if self.msks is None else d[B:2 * B], (B, bands, H, W), mtd=mtd, ids=ids,
                                               keep=(img_u8, msk_raw))
        except BaseException:
            cache.release(items)
            raise
        cache.commit(items)
        return batch

    def __iter__(self):
        if self.cache is not None:
            self.cache.abandon()      # jobs of an earlier iteration that were begun and never finished
        pending = None
        try:
            for idx in epoch_batches(len(self.imgs), self.batch_size, self.shuffle, self.drop_last, self.generator):
                job = self._begin(idx)
                if pending is not None:
                    yield self._finish(pending)
                pending = job
            if pending is not None:
                yield self._finish(pending)
        finally:
            if self.cache is not None:
                self.cache.abandon()
