"""The device read path of mask TIFFs (metrics(decode="device")): the host reads the file bytes and parses the
IFD (``tiff_ifd.Directory``), the compressed strips of a whole chunk of files go up in one copy, one call of ``ops.tiff_lzw_decode``
(csrc/tiff_lzw.hip) decodes every strip of the chunk, and the pixels stay on the device.

``tiff_strip_layout`` accepts the files PIL, libtiff / GDAL and ``writer.tiff_lzw_file`` write for 8-bit single-band masks and
nothing else; every other file, and every file one of whose strips the kernel gives a status other than 0, is decoded by PIL
exactly as ``decode="host"`` does, and that outcome (pixels or exception) is final: the two modes cannot disagree about a file.
``read_masks`` is ``begin_read_masks`` (read, parse, upload, queue the decode) followed by ``finish_read_masks`` (wait for the
chunk's status, fall back where needed); ``metrics`` begins the next chunk before it finishes the current one.
"""
from __future__ import annotations

import os
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass

import numpy as np
import torch

from .tiff_ifd import LONG, SHORT, TAG, Directory, DirectoryError, old_style_lzw
from .tiff_staging import PinnedPair

StripLayout = namedtuple("StripLayout", "H W rows_per_strip offsets counts compression")

MAX_LZW_STRIP = 65536   # decoded bytes of one LZW strip the kernel takes (flair_tiff_lzw_decode_max_strip): PIL's 64 KB strip
READ_THREADS = 8        # file reads of a chunk in flight


def _layout(data) -> StripLayout | None:
    """tiff_strip_layout's policy over the directory: only the tags that decide what the bytes of a strip mean are looked at"""
    def one(tag, default):
        v = d.ints(tag, (SHORT, LONG))
        return default if v is None else v[0] if len(v) == 1 else None

    try:   # DirectoryError: no directory, a value of another type than SHORT or LONG, or one outside the file
        d = Directory(data)
        n, tags = len(data), d.entries
        if d.bigtiff or TAG.TileWidth in tags or TAG.TileLength in tags:
            return None
        W, H = one(TAG.ImageWidth, None), one(TAG.ImageLength, None)
        if not W or not H:
            return None
        compression = one(TAG.Compression, 1)
        # PIL reads an absent PhotometricInterpretation as WhiteIsZero and inverts those pixels, and applies an Orientation: only what
        # it returns as stored is taken here (BlackIsZero, palette indices)
        if (one(TAG.BitsPerSample, 1) != 8 or one(TAG.SamplesPerPixel, 1) != 1 or compression not in (1, 5) or one(TAG.Predictor, 1) != 1 or
                one(TAG.FillOrder, 1) != 1 or one(TAG.PlanarConfiguration, 1) != 1 or one(TAG.PhotometricInterpretation, None) not in (1, 3) or
                one(TAG.Orientation, 1) != 1 or one(TAG.SampleFormat, 1) != 1):
            return None
        rows = one(TAG.RowsPerStrip, H)
        if not rows:
            return None
        rows = min(rows, H)
        offsets, counts = d.ints(TAG.StripOffsets, (SHORT, LONG)), d.ints(TAG.StripByteCounts, (SHORT, LONG))
        nstrips = -(-H // rows)
        if not offsets or not counts or len(offsets) != nstrips or len(counts) != nstrips:
            return None
        if any(off + cnt > n for off, cnt in zip(offsets, counts)):
            return None
        if compression == 5 and (rows * W > MAX_LZW_STRIP or old_style_lzw(data, offsets, counts) is not None):
            return None
        return StripLayout(H, W, rows, offsets, counts, compression)
    except DirectoryError:
        return None


def tiff_strip_layout(data) -> StripLayout | None:
    """(H, W, rows_per_strip, offsets, counts, compression) of a TIFF whose strips ``ops.tiff_lzw_decode`` can take, None for every
    other file (and for bytes that are no TIFF at all; nothing is raised): classic TIFF, II or MM, first IFD, 8 bits, one sample,
    Compression 1 or 5, no predictor, FillOrder 1, chunky, strips (no tiles) with SHORT or LONG offsets and counts inside the file,
    ceil(H / rows_per_strip) of them, LZW strips of at most MAX_LZW_STRIP decoded bytes."""
    try:
        return _layout(data)
    except Exception:  # noqa: BLE001 - foreign bytes: whatever they break, the file is PIL's
        return None


@dataclass
class MaskRead:
    pixels: torch.Tensor | None     # device uint8, (H, W)
    error: Exception | None
    where: str                      # "device" | "host" | "host_after_device_error" | "error"
    buffer: torch.Tensor | None = None   # the flat device buffer the pixels of the call share, where these pixels lie in it
    offset: int = -1                     # their first byte there, a multiple of 16


def _as_u8(a: np.ndarray, truth: bool) -> np.ndarray:
    from .metrics import _as_u8 as f
    return f(a, truth)


def _pil_pixels(path, truth: bool) -> np.ndarray:
    """what metrics(decode="host") makes of the file; raises what it raises"""
    from PIL import Image
    return np.array(_as_u8(np.asarray(Image.open(path)), truth=truth), order="C")   # a writable copy: torch.from_numpy takes it


_pool = None
_staging = PinnedPair()   # taken in turn: one chunk's copy may be in flight while the next chunk is read


def _read_pool():
    global _pool
    if _pool is None:
        _pool = ThreadPoolExecutor(max_workers=READ_THREADS, thread_name_prefix="flair-tiff-read")
    return _pool


def _read_into(args):
    path, view = args
    try:
        with open(path, "rb") as f:
            return f.readinto(view) == len(view) and not f.read(1)
    except OSError:
        return False


def _align16(n):
    return (n + 15) & ~15


class PendingMasks:
    """what begin_read_masks leaves for finish_read_masks: the decode of the chunk is queued, its status not yet read"""

    def __init__(self, paths, flags, device):
        self.paths, self.flags, self.device = paths, flags, device
        self.host = {}       # index -> (array | exception, where): the files PIL decoded
        self.layouts = {}    # index -> StripLayout: the files the kernel decodes
        self.pix_off = {}
        self.pixels = None
        self.status = None   # pinned int32 per strip, valid once the event `decoded` has passed
        self.decoded = None
        self.owner = []      # the file of each strip

    def by_pil(self, i, where):
        try:
            return _pil_pixels(self.paths[i], self.flags[i]), where
        except Exception as e:  # noqa: BLE001 - the host mode's own outcome for this file
            return e, "error"


def begin_read_masks(paths, device, decode="device", truth=False) -> PendingMasks:
    """The first half of read_masks: reads and parses the files, uploads them and queues the decode, without waiting for the device;
    PIL decodes the files outside the subset here.  A caller that begins the next chunk before it finishes this one overlaps this
    chunk's kernel with the next chunk's file reads (metrics does)."""
    paths = [os.fspath(p) for p in paths]
    flags = [bool(truth)] * len(paths) if isinstance(truth, (bool, int)) else [bool(t) for t in truth]
    if len(flags) != len(paths):
        raise ValueError("read_masks: one truth flag per path")
    if decode not in ("host", "device"):
        raise ValueError(f"read_masks decode must be 'host' or 'device', got {decode!r}")
    job = PendingMasks(paths, flags, torch.device(device))
    host, layouts, pix_off = job.host, job.layouts, job.pix_off
    if decode == "device" and paths:
        from . import ops
        sizes = []
        for p in paths:
            try:
                sizes.append(os.stat(p).st_size)
            except OSError:
                sizes.append(-1)
        bases, total = [], 0
        for s in sizes:
            bases.append(total)
            total += _align16(max(s, 0))
        staging, slot = _staging.take_next(total)
        raw = staging.numpy()
        jobs = [(p, memoryview(raw[b:b + s])) for p, b, s in zip(paths, bases, sizes) if s > 0]
        complete = iter(list(_read_pool().map(_read_into, jobs)))
        for i, (b, s) in enumerate(zip(bases, sizes)):
            lay = tiff_strip_layout(raw[b:b + s]) if s > 0 and next(complete) else None
            if lay is None:
                host[i] = job.by_pil(i, "host")
            else:
                layouts[i] = lay
    else:
        for i in range(len(paths)):
            host[i] = job.by_pil(i, "host")

    # the pixel buffer: every file with a known size, in path order
    pix_total = 0
    for i in range(len(paths)):
        n = layouts[i].H * layouts[i].W if i in layouts else (host[i][0].size if isinstance(host[i][0], np.ndarray) else 0)
        if n:
            pix_off[i] = pix_total
            pix_total = _align16(pix_total + n)
    job.pixels = torch.empty(max(pix_total, 1), dtype=torch.uint8, device=job.device)

    if layouts:
        src_off, src_len, dst_off, dst_len, mode = [], [], [], [], []
        for i, lay in layouts.items():
            strip_bytes = lay.rows_per_strip * lay.W
            for k, (off, cnt) in enumerate(zip(lay.offsets, lay.counts)):
                src_off.append(bases[i] + off)
                src_len.append(cnt)
                dst_off.append(pix_off[i] + k * strip_bytes)
                dst_len.append(min(strip_bytes, lay.H * lay.W - k * strip_bytes))
            mode += [1 if lay.compression == 5 else 0] * len(lay.offsets)
            job.owner += [i] * len(lay.offsets)
        # the five tables in two small copies: [src_off | dst_off] int64, [src_len | dst_len | mode] int32
        t64 = torch.tensor([src_off, dst_off], dtype=torch.int64).to(job.device)
        t32 = torch.tensor([src_len, dst_len, mode], dtype=torch.int32).to(job.device)
        src = staging[:total].to(job.device, non_blocking=True)
        _staging.copied(slot)
        _, status = ops.tiff_lzw_decode(src, t64[0], t32[0], t64[1], t32[1], t32[2], job.pixels.numel(), out=job.pixels)
        # the status comes down behind this chunk's kernel, ahead of whatever the caller queues next
        job.status = torch.empty(status.shape, dtype=torch.int32, pin_memory=True)
        job.status.copy_(status, non_blocking=True)
        job.decoded = torch.cuda.Event()
        job.decoded.record()
    return job


def finish_read_masks(job: PendingMasks) -> list:
    """The second half: waits for the chunk's status, hands the files with a strip status other than 0 to PIL, returns the MaskReads"""
    paths, host, layouts, pix_off, pixels = job.paths, job.host, job.layouts, job.pix_off, job.pixels
    if job.status is not None:
        job.decoded.synchronize()
        status = job.status.numpy()
        for i in sorted(set(np.asarray(job.owner)[status != 0].tolist())):
            host[i] = job.by_pil(i, "host_after_device_error")
    out = [None] * len(paths)
    for i in range(len(paths)):
        if i in host:
            got, where = host[i]
            if isinstance(got, Exception):
                out[i] = MaskRead(None, got, "error")
                continue
            flat = torch.from_numpy(got.reshape(-1))
            if i in pix_off and (i not in layouts or got.size == layouts[i].H * layouts[i].W):
                view = pixels[pix_off[i]:pix_off[i] + got.size]
                view.copy_(flat)
                out[i] = MaskRead(view.view(got.shape), None, where, pixels, pix_off[i])
            else:   # a file PIL sees at another size than its IFD says
                out[i] = MaskRead(flat.to(job.device).view(got.shape), None, where)
        else:
            lay = layouts[i]
            out[i] = MaskRead(pixels[pix_off[i]:pix_off[i] + lay.H * lay.W].view(lay.H, lay.W), None, "device", pixels, pix_off[i])
    return out


def read_masks(paths, device, decode="device", truth=False) -> list:
    """One MaskRead per path.  ``truth`` (one bool, or one per path) only matters to files PIL decodes: it picks the byte that values
    outside 0 .. 255 of a wider raster become (metrics._as_u8).  With ``decode="device"`` the pixels of all files of the call share one
    device buffer, in path order, each file's starting at a multiple of 16 bytes: files of a multiple of 16 pixels are contiguous."""
    return finish_read_masks(begin_read_masks(paths, device, decode, truth))
