"""The file zone_detect starts from (reference src/zone_detect/main.py, ``input_img_path``): a multi-band 8-bit orthophoto TIFF, read
into the (bands, H, W) uint8 device tensor ``ZoneDetector.run`` takes.  The host parses the first IFD (``raster_layout``, a policy
over ``tiff_ifd.Directory``) and reads the compressed chunks, the tiles or strips of the file, group by group into pinned memory; the
device decodes them (``ops.tiff_lzw_decode_chunks``, csrc/tiff_read.hip: stored or LZW, one wave per chunk, any chunk size up to
``CHUNK_CAP``) and scatters them into the band planes with the horizontal predictor undone (``ops.tiff_chunks_to_planes``).  Only
compressed bytes cross PCIe.  This is the family of files ``raster_writer.write_raster`` and GDAL (``COMPRESS=LZW``, ``PREDICTOR=2``,
``INTERLEAVE=BAND`` / ``PIXEL``, tiled or striped) write; DESIGN §10 has the layout.  There is no fallback reader: a file outside the
family is refused by name (``UnsupportedRaster``), because nothing else in the package reads a 5-band file either.
"""
from __future__ import annotations

import mmap
import os
from dataclasses import dataclass

import numpy as np
import torch

from .tiff_ifd import BYTE, INT_FORMAT, TAG, TAG_NAMES, TYPE_SIZE, Directory, DirectoryError, old_style_lzw
from .tiff_staging import GROUP_BYTES, PinnedPair, stream_groups

CHUNK_CAP = 1 << 24      # decoded bytes of one LZW chunk the kernel takes (flair_tiff_lzw_decode_chunks_cap)
CHUNK_WINDOW = 12288     # the decoder's LDS window of recent output (flair_tiff_lzw_decode_chunks_window): older sources are read back
FLUSH_BLOCK = 128        # ... from the slot, which is written in whole blocks of this size; slots are multiples of it
MERGE_GAP = 1 << 16      # chunks of a group that lie this close in the file are read with one read()

STATUS_TEXT = {1: "the compressed bytes ran out", 2: "EOI came before the chunk was complete", 3: "a table code first after a clear",
               4: "a code the table does not hold", 5: "a range or cap error"}


class UnsupportedRaster(ValueError):
    """the file is no TIFF of the family raster_layout accepts; the message names the tag and its value"""


class RasterDecodeError(RuntimeError):
    """a chunk of the file did not decode; ``chunk`` is its index in the file's offset array, ``status`` the kernel's code"""

    def __init__(self, message, chunk, status):
        super().__init__(message)
        self.chunk, self.status = chunk, status


_NO_DIRECTORY = {"order": "not a TIFF: the file does not begin with II or MM", "magic": "not a TIFF: magic number {magic}",
                 "ifd": "the IFD at {ifd} lies outside the file of {n} bytes",
                 "entries": "the IFD at {ifd} with {count} entries lies outside the file of {n} bytes"}   # by DirectoryError.what


def _name(tag):
    return f"{TAG_NAMES.get(tag, 'tag')} ({tag})"


@dataclass(frozen=True)
class RasterLayout:
    """What the bytes of a file's chunks mean.  ``chunk_w`` x ``chunk_h``: TileWidth x TileLength, or ImageWidth x RowsPerStrip for
    strips; ``offsets`` / ``counts``: int64 arrays in the file's chunk order, band-major for ``planar`` 2."""
    H: int
    W: int
    bands: int
    planar: int
    compression: int
    predictor: int
    tiled: bool
    chunk_w: int
    chunk_h: int
    offsets: np.ndarray
    counts: np.ndarray
    bigtiff: bool
    order: str

    @property
    def samples(self) -> int:
        """bytes per pixel of a decoded chunk"""
        return self.bands if self.planar == 1 else 1

    @property
    def chunks_x(self) -> int:
        return -(-self.W // self.chunk_w)

    @property
    def chunks_y(self) -> int:
        return -(-self.H // self.chunk_h)

    @property
    def n_chunks(self) -> int:
        return (1 if self.planar == 1 else self.bands) * self.chunks_y * self.chunks_x

    def chunk_table(self) -> np.ndarray:
        """(n_chunks, 5) int32 rows {x0, y0, width, rows, band0} as flair_tiff_chunks_to_planes takes them: tiles are full size, the
        last strip is short"""
        cy, cx = self.chunks_y, self.chunks_x
        i = np.arange(self.n_chunks, dtype=np.int64)
        band0, y, x = i // (cy * cx), (i // cx) % cy, i % cx
        y0 = y * self.chunk_h
        rows = np.full_like(i, self.chunk_h) if self.tiled else np.minimum(self.chunk_h, self.H - y0)
        return np.stack([x * self.chunk_w, y0, np.full_like(i, self.chunk_w), rows, band0], axis=1).astype(np.int32)

    @property
    def slot_bytes(self) -> int:
        """a decoded chunk rounded up to the decoder's flush block: the slot a chunk of this file needs"""
        return -(-self.chunk_w * self.chunk_h * self.samples // FLUSH_BLOCK) * FLUSH_BLOCK

    def decode_tables(self):
        """(table, src_len, dst_len, mode): ``chunk_table()`` and the three int32 arrays flair_tiff_lzw_decode_chunks takes next to
        the source offsets: the compressed and the decoded bytes of every chunk, and 0 = stored / 1 = LZW"""
        table = self.chunk_table()
        dst_len = (table[:, 2].astype(np.int64) * table[:, 3] * self.samples).astype(np.int32)
        mode = np.full(self.n_chunks, 1 if self.compression == 5 else 0, dtype=np.int32)
        return table, self.counts.astype(np.int32), dst_len, mode

    def chunk_name(self, i: int) -> str:
        x0, y0, _, _, band0 = self.chunk_table()[i]
        kind = "tile" if self.tiled else "strip"
        band = f", band {band0}" if self.planar == 2 else ""
        return f"chunk {i} ({kind} at row {y0}, column {x0}{band})"


def raster_layout(data) -> RasterLayout:
    """The layout of the first IFD of ``data`` (bytes, a memoryview or an mmap of the whole file), or ``UnsupportedRaster``.
    Accepted: classic TIFF and BigTIFF, II and MM; 8-bit unsigned samples, any number of bands (ExtraSamples and
    PhotometricInterpretation are ignored: the bytes are returned as stored); Compression 1 or 5, Predictor 1 or 2 (2 with LZW only),
    FillOrder 1, Orientation 1, PlanarConfiguration 1 or 2; tiles whose sides are multiples of 16, or strips of any RowsPerStrip;
    offsets and counts as SHORT, LONG or LONG8, in exactly the expected number, all inside the file."""
    n = len(data)
    try:
        d = Directory(data)
        if d.end + d.inline > n:   # the offset of the next IFD belongs to this one
            raise DirectoryError("entries", ifd=d.ifd, count=d.count)
    except DirectoryError as err:
        raise UnsupportedRaster(_NO_DIRECTORY[err.what].format(n=n, **vars(err))) from None
    tags = d.entries

    def values(tag):
        """the entry's integers as an array, None when it is absent"""
        try:
            v = d.ints(tag, INT_FORMAT)
        except DirectoryError as err:
            typ, cnt, _ = tags[tag]
            if err.what == "type":
                raise UnsupportedRaster(f"{_name(tag)} has type {typ} and count {cnt}, not BYTE, SHORT, LONG or LONG8 values") from None
            raise UnsupportedRaster(f"the {cnt} values of {_name(tag)} at {err.at} lie outside the file of {n} bytes") from None
        return None if v is None else np.array(v, dtype=f"u{TYPE_SIZE[tags[tag][0]]}")

    def one(tag, default):
        v = values(tag)
        if v is None:
            if default is None:
                raise UnsupportedRaster(f"{_name(tag)} is missing")
            return default
        if len(v) != 1:
            raise UnsupportedRaster(f"{_name(tag)} holds {len(v)} values, expected one")
        return int(v[0])

    def all_equal(tag, want, default_ok, bands):
        v = values(tag)
        if v is None:
            if not default_ok:
                raise UnsupportedRaster(f"{_name(tag)} is missing (its default is not {want})")
            return
        if len(v) != bands or (v != want).any():
            raise UnsupportedRaster(f"{_name(tag)} is {[int(x) for x in v[:8]]}, expected {want} for each of the {bands} samples")

    W, H = one(TAG.ImageWidth, None), one(TAG.ImageLength, None)
    if not 1 <= W < 1 << 31:
        raise UnsupportedRaster(f"{_name(TAG.ImageWidth)} is {W}")
    if not 1 <= H < 1 << 31:
        raise UnsupportedRaster(f"{_name(TAG.ImageLength)} is {H}")
    subfile = one(TAG.NewSubfileType, 0)
    if subfile & 5:
        raise UnsupportedRaster(f"{_name(TAG.NewSubfileType)} is {subfile}: the first IFD is a reduced-resolution image or a mask, not the raster")
    bands = one(TAG.SamplesPerPixel, 1)
    if bands < 1:
        raise UnsupportedRaster(f"{_name(TAG.SamplesPerPixel)} is {bands}")
    all_equal(TAG.BitsPerSample, 8, False, bands)
    all_equal(TAG.SampleFormat, 1, True, bands)
    compression = one(TAG.Compression, 1)
    if compression not in (1, 5):
        raise UnsupportedRaster(f"{_name(TAG.Compression)} is {compression}: only 1 (stored) and 5 (LZW) are read")
    predictor = one(TAG.Predictor, 1)
    if predictor not in (1, 2) or (predictor == 2 and compression == 1):
        raise UnsupportedRaster(f"{_name(TAG.Predictor)} is {predictor} with Compression {compression}: 1, or 2 with LZW, are read")
    for tag in (TAG.FillOrder, TAG.Orientation):
        v = one(tag, 1)
        if v != 1:
            raise UnsupportedRaster(f"{_name(tag)} is {v}, expected 1")
    planar = one(TAG.PlanarConfiguration, 1)
    if planar not in (1, 2):
        raise UnsupportedRaster(f"{_name(TAG.PlanarConfiguration)} is {planar}, expected 1 or 2")
    if bands == 1:
        planar = 1   # the two mean the same bytes
    tiled = TAG.TileWidth in tags or TAG.TileLength in tags
    if tiled:
        cw, ch = one(TAG.TileWidth, None), one(TAG.TileLength, None)
        for tag, v in ((TAG.TileWidth, cw), (TAG.TileLength, ch)):
            if v < 16 or v % 16 or v >= 1 << 31:
                raise UnsupportedRaster(f"{_name(tag)} is {v}, no positive multiple of 16")
        off_tag, cnt_tag = TAG.TileOffsets, TAG.TileByteCounts
    else:
        cw, ch = W, min(one(TAG.RowsPerStrip, (1 << 32) - 1), H)
        if ch < 1:
            raise UnsupportedRaster(f"{_name(TAG.RowsPerStrip)} is {ch}")
        off_tag, cnt_tag = TAG.StripOffsets, TAG.StripByteCounts
    samples = bands if planar == 1 else 1
    chunk_bytes = cw * ch * samples
    if chunk_bytes >= 1 << 31 or (compression == 5 and chunk_bytes > CHUNK_CAP):
        raise UnsupportedRaster(f"{_name(TAG.TileLength if tiled else TAG.RowsPerStrip)} makes chunks of {cw} x {ch} x {samples} = "
                                f"{chunk_bytes} bytes, more than the decoder's {CHUNK_CAP}")
    n_chunks = (1 if planar == 1 else bands) * -(-H // ch) * -(-W // cw)
    offsets, counts = values(off_tag), values(cnt_tag)
    for tag, v in ((off_tag, offsets), (cnt_tag, counts)):
        if v is None:
            raise UnsupportedRaster(f"{_name(tag)} is missing")
        if tags[tag][0] == BYTE or len(v) != n_chunks:
            raise UnsupportedRaster(f"{_name(tag)} holds {len(v)} values of type {tags[tag][0]}, expected {n_chunks} SHORT, LONG or LONG8")
    offsets, counts = offsets.astype(np.int64), counts.astype(np.int64)
    if (offsets < 0).any() or (counts < 0).any() or (counts >= 1 << 31).any():
        raise UnsupportedRaster(f"{_name(cnt_tag)} holds a count of 2^31 bytes or more")
    outside = np.flatnonzero((offsets < 8) | (offsets + counts > n))
    if len(outside):
        i = int(outside[0])
        raise UnsupportedRaster(f"{_name(off_tag)}: chunk {i} at [{int(offsets[i])}, + {int(counts[i])}) lies outside the file of {n} bytes")
    old = old_style_lzw(data, offsets.tolist(), counts.tolist()) if compression == 5 else None
    if old is not None:
        raise UnsupportedRaster(f"{_name(TAG.Compression)} is 5, but chunk {old} is an old-style (LSB-first) LZW stream")
    return RasterLayout(H, W, bands, planar, compression, predictor, tiled, cw, ch, offsets, counts, d.bigtiff, d.order)


def read_plan(layout: RasterLayout, group_bytes: int = GROUP_BYTES):
    """How read_raster goes through the file: (groups, slot_bytes, src_off, reads).  ``groups``: (first, n) chunk windows whose slots
    fit ``group_bytes`` (whole chunk rows where they fit, ``raster_writer.stream_groups``); ``slot_bytes``: a decoded chunk rounded up to
    the flush block; ``src_off[i]``: where chunk i lies in its group's staging buffer; ``reads[g]``: (buffer bytes, [(file offset,
    length, buffer offset)]) - chunks are read in file order and neighbours closer than ``MERGE_GAP`` with one read()."""
    slot = layout.slot_bytes
    groups = stream_groups(layout.n_chunks, layout.chunks_x, slot, group_bytes)
    src_off = np.zeros(layout.n_chunks, dtype=np.int64)
    reads = []
    for first, n in groups:
        off, cnt = layout.offsets[first:first + n], layout.counts[first:first + n]
        runs, at = [], 0
        run_lo = run_hi = None
        for i in np.argsort(off, kind="stable"):
            o, c = int(off[i]), int(cnt[i])
            if run_lo is None or o > run_hi + MERGE_GAP:
                if run_lo is not None:
                    runs.append((run_lo, run_hi - run_lo, at))
                    at += -(-(run_hi - run_lo) // 16) * 16
                run_lo, run_hi = o, o + c
            src_off[first + i] = at + (o - run_lo)
            run_hi = max(run_hi, o + c)
        runs.append((run_lo, run_hi - run_lo, at))
        reads.append((at + run_hi - run_lo, runs))
    return groups, slot, src_off, reads


_staging = PinnedPair()   # read_raster's own, kept between calls


def _read_runs(f, runs, staging):
    view = memoryview(staging.numpy())
    for file_off, length, at in runs:
        f.seek(file_off)
        got = f.readinto(view[at:at + length])
        if got != length:
            raise OSError(f"short read: {got} of {length} bytes at {file_off}")


def read_raster(path, device, group_bytes: int = GROUP_BYTES) -> torch.Tensor:
    """The (bands, H, W) uint8 raster of a TIFF, on ``device``.  The chunks are worked through in groups whose decoded bytes fit
    ``group_bytes``: the group's file ranges are read into one of two pinned buffers, go up in one copy on a side stream, are decoded
    into the group's slots and scattered into the planes; the host reads the next group while the device decodes the current one.
    One wait at the end fetches every chunk's status; ``RasterDecodeError`` names the first chunk whose status is not 0.  Stored
    chunks take the same path (mode 0).  The memory next to the raster is bounded by the group."""
    from . import ops
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("read_raster decodes on the HIP device")
    with open(path, "rb") as f:
        if os.fstat(f.fileno()).st_size < 8:
            raise UnsupportedRaster("not a TIFF: fewer than 8 bytes")
        with mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as mm:
            layout = raster_layout(mm)
        groups, slot, src_off, reads = read_plan(layout, group_bytes)
        table, src_len, dst_len, mode = layout.decode_tables()
        with torch.cuda.device(dev):
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
            d_src_off, d_src_len, d_dst_len, d_mode, d_table = up(src_off), up(src_len), up(dst_len), up(mode), up(table)
            status = torch.empty(layout.n_chunks, dtype=torch.int32, device=dev)
            planes = torch.empty(layout.bands, layout.H, layout.W, dtype=torch.uint8, device=dev)
            scratch = torch.empty(max(n for _, n in groups) * slot, dtype=torch.uint8, device=dev)
            src_max = max(nbytes for nbytes, _ in reads)
            d_src = [torch.empty(max(src_max, 16), dtype=torch.uint8, device=dev) for _ in range(min(2, len(groups)))]
            main, copy_stream = torch.cuda.current_stream(), torch.cuda.Stream(device=dev)
            uploaded, decoded = [None, None], [None, None]
            try:
                for g, ((first, n), (nbytes, runs)) in enumerate(zip(groups, reads)):
                    k = g & 1
                    if uploaded[k] is not None:
                        uploaded[k].synchronize()        # the pinned buffer's last copy has left it
                    staging = _staging.take(k, nbytes)
                    _read_runs(f, runs, staging)
                    if decoded[k] is not None:
                        copy_stream.wait_event(decoded[k])   # the device buffer's last decode has read it
                    with torch.cuda.stream(copy_stream):
                        d_src[k][:nbytes].copy_(staging[:nbytes], non_blocking=True)
                        uploaded[k] = torch.cuda.Event()
                        uploaded[k].record()
                    main.wait_event(uploaded[k])
                    sl = slice(first, first + n)
                    slots, st = ops.tiff_lzw_decode_chunks(d_src[k][:max(nbytes, 1)], d_src_off[sl], d_src_len[sl], d_dst_len[sl], d_mode[sl],
                                                           slot, out=scratch[:n * slot], status=status[sl])
                    ops.tiff_chunks_to_planes(slots, d_table[sl], st, planes, layout.samples, layout.predictor, max_rows=layout.chunk_h)
                    decoded[k] = torch.cuda.Event()
                    decoded[k].record()
            finally:
                copy_stream.synchronize()   # no buffer is freed under a copy
            status_h = status.cpu().numpy()   # the one wait
    raise_if_failed(path, layout, status_h)
    return planes


def raise_if_failed(path, layout: RasterLayout, status):
    """``RasterDecodeError`` for the first chunk of the file whose status (one code per chunk, in the file's chunk order) is not 0"""
    bad = np.flatnonzero(status)
    if len(bad):
        i = int(bad[0])
        code = int(status[i])
        raise RasterDecodeError(f"{os.fspath(path)!r}: {layout.chunk_name(i)} did not decode: status {code} "
                                f"({STATUS_TEXT.get(code, 'unknown')}); {len(bad)} of {layout.n_chunks} chunks failed", i, code)
