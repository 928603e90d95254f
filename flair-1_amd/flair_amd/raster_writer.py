"""The file zone_detect ends in (reference src/zone_detect/main.py:206-232, :386-428): one tiled, LZW-compressed TIFF of the output
raster, BigTIFF by default, tiles of ``img_pixels_detection``, 2 bands (class, confidence byte) for ``output_type: argmax`` or
``n_classes`` bands for ``class_prob``.  The raster stays on the device: ``ops.tiff_lzw_encode_tiles`` (csrc/tiff_lzw.hip) makes one
LZW stream per TIFF tile, ``ops.tiff_pack_streams`` packs the streams of a group back to back, and only those bytes cross PCIe,
into one of two pinned buffers on a side stream, while the next group is encoded and a worker thread appends the previous one to
the file.  The host frames (``tiled_tiff_header``, ``tiled_tiff_ifd`` over ``tiff_ifd.build_ifd``) and calls ``write()``; DESIGN §10.

``read_geo_tags`` lifts the GeoTIFF tags of the source raster as raw bytes (``tiff_ifd.Directory.raw_le``) and
``tiled_tiff_ifd(geo_tags=...)`` puts them into the output, so the result overlays its input (what ``profile.copy()`` does in the
reference's ``prepare_output``); nothing here interprets them, and rasterio is not involved.
"""
from __future__ import annotations

import mmap
import os
import queue
import struct
import threading

import numpy as np
import torch

from .tiff_ifd import LONG, LONG8, SHORT, TAG, TYPE_SIZE, Directory, DirectoryError, build_ifd, entry
from .tiff_staging import GROUP_BYTES, PinnedPair, stream_groups  # noqa: F401 - both names stay importable from here

INTERLEAVE = ("band", "pixel")     # PlanarConfiguration 2 / 1, GDAL's INTERLEAVE=BAND / PIXEL
GEO_TAGS = (33550, 33922, 34264, 34735, 34736, 34737, 42113)   # pixel scale, tiepoints, transformation, key directory, double and
#                                                                 ASCII parameters, GDAL_NODATA
DATA_START = 16                    # where the first stream lies: the BigTIFF header's size, the classic header's rounded up to 16


def _check_layout(H, W, bands, tile, interleave):
    if interleave not in INTERLEAVE:
        raise ValueError(f"interleave must be 'band' or 'pixel', got {interleave!r}")
    if int(tile) < 16 or int(tile) % 16:
        raise ValueError(f"tile must be a positive multiple of 16 (TIFF 6.0, section 15), got {tile}")
    if H < 1 or W < 1 or bands < 1:
        raise ValueError(f"a raster of {bands} x {H} x {W} has no pixel")
    return (1 if interleave == "pixel" else bands) * -(-H // tile) * -(-W // tile)


def tiled_tiff_header(ifd_offset: int, bigtiff: bool = True) -> bytes:
    """The little-endian file header that points at the IFD: 16 bytes (BigTIFF) or 8 (classic TIFF)."""
    if bigtiff:
        return struct.pack("<2sHHHQ", b"II", 43, 8, 0, ifd_offset)
    if ifd_offset >= 1 << 32:
        raise ValueError(f"a classic TIFF cannot place its IFD at {ifd_offset}: use bigtiff=True")
    return struct.pack("<2sHI", b"II", 42, ifd_offset)


def tiled_tiff_ifd(H: int, W: int, bands: int, tile: int, interleave: str, offsets, counts, ifd_offset: int, bigtiff: bool = True,
                   geo_tags=None) -> bytes:
    """The one IFD of a tiled 8-bit LZW TIFF of ``bands`` samples, followed by the arrays that do not fit its entries, as it must lie at
    ``ifd_offset``.  ``offsets`` / ``counts``: where each tile's stream lies in the file and how long it is, in the stream order of
    ``ops.tiff_lzw_encode_tiles``.  ``geo_tags``: {tag: (type, count, little-endian bytes)} as ``read_geo_tags`` returns them."""
    H, W, bands, tile, ifd_offset = int(H), int(W), int(bands), int(tile), int(ifd_offset)
    n = _check_layout(H, W, bands, tile, interleave)
    offsets, counts = [int(v) for v in offsets], [int(v) for v in counts]
    if len(offsets) != n or len(counts) != n:
        raise ValueError(f"{len(offsets)} offsets and {len(counts)} counts for {n} tiles")
    if ifd_offset < 8 or ifd_offset % 2:
        raise ValueError(f"an IFD cannot lie at {ifd_offset}")
    planar = 2 if interleave == "band" and bands > 1 else 1
    if not bigtiff and max(o + c for o, c in zip(offsets, counts)) > 1 << 32:
        raise ValueError("a classic TIFF holds offsets below 2^32 only: use bigtiff=True")
    wide = LONG8 if bigtiff else LONG
    # what GDAL makes of 8-bit bands, and what libtiff-based readers need to see every band: three are RGB, of any other number
    # the first is grey and the others are extra samples of unspecified meaning
    rgb = bands == 3
    entries = [entry(TAG.ImageWidth, LONG, [W]), entry(TAG.ImageLength, LONG, [H]), entry(TAG.BitsPerSample, SHORT, [8] * bands),
               entry(TAG.Compression, SHORT, [5]), entry(TAG.PhotometricInterpretation, SHORT, [2 if rgb else 1]),
               entry(TAG.SamplesPerPixel, SHORT, [bands]), entry(TAG.PlanarConfiguration, SHORT, [planar]),
               entry(TAG.TileWidth, LONG, [tile]), entry(TAG.TileLength, LONG, [tile]),
               entry(TAG.TileOffsets, wide, offsets), entry(TAG.TileByteCounts, wide, counts),
               entry(TAG.SampleFormat, SHORT, [1] * bands)]
    if bands > 1 and not rgb:
        entries.append(entry(TAG.ExtraSamples, SHORT, [0] * (bands - 1)))
    for tag, (typ, cnt, raw) in (geo_tags or {}).items():
        tag, typ, cnt, raw = int(tag), int(typ), int(cnt), bytes(raw)
        if tag not in GEO_TAGS or typ not in TYPE_SIZE or len(raw) != TYPE_SIZE[typ] * cnt:
            raise ValueError(f"geo tag {tag}: type {typ}, count {cnt}, {len(raw)} bytes")
        entries.append((tag, typ, cnt, raw))
    return build_ifd(sorted(entries, key=lambda e: e[0]), ifd_offset, bigtiff, align=8)


def read_geo_tags(path) -> dict:
    """{tag: (type, count, value bytes)} of the GeoTIFF tags (``GEO_TAGS``) in the first IFD of a classic or BigTIFF file, ``{}`` when
    it has none; the bytes are the file's own, in little-endian order (those of a big-endian file are swapped per value, nothing is
    interpreted).  ValueError for bytes that are no TIFF."""
    name = os.fspath(path)
    with open(path, "rb") as f:
        if os.fstat(f.fileno()).st_size < 8:
            raise ValueError(f"{name!r} is not a TIFF")
        with mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
            try:
                d = Directory(mm)
                return {tag: d.raw_le(tag) for tag, (typ, _, _) in d.entries.items() if tag in GEO_TAGS and typ in TYPE_SIZE}
            except DirectoryError as err:
                if err.what in ("order", "magic"):
                    raise ValueError(f"{name!r} is not a TIFF") from None
                where = f"tag {err.tag}" if err.what == "outside" else "the IFD"
                raise ValueError(f"{name!r}: {where} lies outside the file") from None


_staging = PinnedPair()   # write_raster's own, kept between calls


def write_raster(path, raster, tile, interleave="band", scale=None, bigtiff=True, geo_tags=None, group_bytes=GROUP_BYTES) -> dict:
    """Writes a (bands, H, W) device raster, uint8 or float32 with a ``scale`` per band (``ops.tiff_lzw_encode_tiles``), as one tiled LZW
    TIFF: header, the streams in stream order, each at a multiple of 16, the IFD and its arrays last.  The streams are encoded, packed
    and brought down in groups of at most ``group_bytes`` raw bytes, so the memory next to the raster is bounded by the group; the
    file's bytes do not depend on the grouping.  Per group the host waits once, for the group's stream lengths.  Returns
    {"file_bytes", "payload_bytes", "streams", "groups"}."""
    from . import ops
    if not torch.is_tensor(raster) or raster.dim() != 3 or not raster.is_cuda:
        raise RuntimeError("write_raster needs a (bands, H, W) tensor on the HIP device")
    bands, H, W = raster.shape
    tile = int(tile)
    n_streams = _check_layout(H, W, bands, tile, interleave)
    raster = raster.contiguous()
    dev = raster.device
    if scale is not None and not torch.is_tensor(scale):
        scale = torch.tensor([float(v) for v in scale], dtype=torch.float32).to(dev)
    samples = bands if interleave == "pixel" else 1
    slot = ops.tiff_lzw_tile_slot_bytes(tile, samples)
    groups = stream_groups(n_streams, -(-W // tile), tile * tile * samples, group_bytes)
    payload = torch.empty(max(n for _, n in groups) * slot, dtype=torch.uint8, device=dev)
    copy_stream = torch.cuda.Stream(device=dev)
    jobs, free, errors = queue.Queue(), queue.Queue(), []
    free.put(0)
    free.put(1)

    def append_groups(f):   # the worker: waits for a group's copy, appends it, hands its buffer back
        while True:
            job = jobs.get()
            if job is None:
                return
            k, nbytes, copied = job
            try:
                if not errors:
                    copied.synchronize()
                    f.write(_staging.buffers[k].numpy()[:nbytes])
            except Exception as e:  # noqa: BLE001 - surfaces from write_raster below
                errors.append(e)
            finally:
                free.put(k)

    all_counts, copied = [], None
    with open(path, "wb") as f:
        f.write(b"\0" * DATA_START)   # the header's place: written last, once the IFD's offset is known
        worker = threading.Thread(target=append_groups, args=(f,), name="flair-raster-write")
        worker.start()
        try:
            for first, n in groups:
                slots, counts = ops.tiff_lzw_encode_tiles(raster, tile, interleave, scale, first, n)
                if copied is not None:   # the one packed buffer is still being read by the previous group's copy
                    torch.cuda.current_stream().wait_event(copied)
                ops.tiff_pack_streams(slots, counts, slot, out=payload)
                counts_h = counts.cpu().numpy().astype(np.int64)   # the group's one wait
                nbytes = int(((counts_h + 15) & ~15).sum())
                k = free.get()   # blocks while both buffers are waiting to be written
                if errors:
                    break
                staging = _staging.take(k, nbytes)
                copy_stream.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(copy_stream):
                    staging[:nbytes].copy_(payload[:nbytes], non_blocking=True)
                    copied = torch.cuda.Event()
                    copied.record()
                jobs.put((k, nbytes, copied))
                all_counts.append(counts_h)
        finally:
            jobs.put(None)
            worker.join()
            copy_stream.synchronize()   # `payload` is not freed under a copy
        if errors:
            raise errors[0]
        counts_h = np.concatenate(all_counts)
        rounded = (counts_h + 15) & ~15
        offsets = DATA_START + np.cumsum(rounded) - rounded
        ifd_offset = DATA_START + int(rounded.sum())
        ifd = tiled_tiff_ifd(H, W, bands, tile, interleave, offsets, counts_h, ifd_offset, bigtiff, geo_tags)
        f.write(ifd)
        f.seek(0)
        f.write(tiled_tiff_header(ifd_offset, bigtiff))
    return {"file_bytes": ifd_offset + len(ifd), "payload_bytes": int(counts_h.sum()), "streams": n_streams, "groups": len(groups)}
