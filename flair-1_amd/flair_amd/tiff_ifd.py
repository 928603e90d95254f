"""The TIFF image file directory, read and written once for every TIFF path of the package: ``Directory`` walks the first
IFD of classic TIFF and BigTIFF bytes of either byte order, ``build_ifd`` lays one out.  Nothing here decides which files are read:
``tiff._layout`` (metrics' masks: None for a file that is PIL's), ``raster_reader.raster_layout`` (zone_detect's input: ``UnsupportedRaster``
by tag name) and ``raster_writer.read_geo_tags`` (ValueError) are policies over a ``Directory``, each with its own acceptance rules and
way of failing; ``writer.tiff_lzw_file`` and ``raster_writer.tiled_tiff_ifd`` say which entries a file has.  No torch, no device."""
import struct
from types import SimpleNamespace

import numpy as np

BYTE, ASCII, SHORT, LONG, RATIONAL, SRATIONAL, LONG8 = 1, 2, 3, 4, 5, 10, 16
TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 13: 4, 16: 8, 17: 8, 18: 8}
UNIT_SIZE = {**TYPE_SIZE, RATIONAL: 4, SRATIONAL: 4}   # what is byte-swapped as one unit: a RATIONAL is two LONGs
INT_FORMAT = {BYTE: "B", SHORT: "H", LONG: "I", LONG8: "Q"}
TAG_NAMES = {254: "NewSubfileType", 256: "ImageWidth", 257: "ImageLength", 258: "BitsPerSample", 259: "Compression",
             262: "PhotometricInterpretation", 266: "FillOrder", 273: "StripOffsets", 274: "Orientation", 277: "SamplesPerPixel",
             278: "RowsPerStrip", 279: "StripByteCounts", 284: "PlanarConfiguration", 317: "Predictor", 322: "TileWidth",
             323: "TileLength", 324: "TileOffsets", 325: "TileByteCounts", 338: "ExtraSamples", 339: "SampleFormat"}
TAG = SimpleNamespace(**{name: tag for tag, name in TAG_NAMES.items()})   # TAG.ImageWidth == 256


class DirectoryError(ValueError):
    """``what``: "order" (no II / MM in 8 bytes), "magic", "ifd" (the entry count lies outside the bytes), "entries" (the entry table
    does), "type" (an entry's type or count is not taken), "outside" (its values lie outside the bytes); plus the fields a message names"""

    def __init__(self, what, **fields):
        super().__init__(what)
        self.what = what
        self.__dict__.update(fields)


class Directory:
    """The first IFD of ``data``.  ``order``: "<" or ">"; ``bigtiff``; ``ifd``: its offset; ``count`` entries; ``end``: the offset behind
    the last, where the offset of the next IFD lies (``inline`` bytes, not looked at); ``entries``: {tag: (type, count, offset of the
    value field)} in file order, the last of two entries of one tag."""

    def __init__(self, data):
        self.data, n = data, len(data)
        mark = bytes(data[:2])
        if n < 8 or mark not in (b"II", b"MM"):
            raise DirectoryError("order")
        self.order = e = "<" if mark == b"II" else ">"
        (magic,) = struct.unpack_from(e + "H", data, 2)
        self.bigtiff = magic == 43
        if magic != 42 and not (self.bigtiff and n >= 16 and struct.unpack_from(e + "HH", data, 4) == (8, 0)):
            raise DirectoryError("magic", magic=magic)
        count_fmt, entry_fmt, entry_size, self.inline, self._offset = ("Q", "HHQ", 20, 8, "Q") if self.bigtiff else ("H", "HHI", 12, 4, "I")
        (self.ifd,) = struct.unpack_from(e + self._offset, data, 8 if self.bigtiff else 4)
        first = self.ifd + struct.calcsize(count_fmt)
        if self.ifd < 8 or first > n:
            raise DirectoryError("ifd", ifd=self.ifd)
        (self.count,) = struct.unpack_from(e + count_fmt, data, self.ifd)
        self.end = first + entry_size * self.count
        if self.end > n:
            raise DirectoryError("entries", ifd=self.ifd, count=self.count)
        table = struct.iter_unpack(f"{e}{entry_fmt}{self.inline}x", data[first:self.end])
        self.entries = {tag: (typ, cnt, first + entry_size * (i + 1) - self.inline) for i, (tag, typ, cnt) in enumerate(table)}

    def _values_at(self, tag, size):
        at = self.entries[tag][2]             # in the entry, or at the offset it holds
        if size > self.inline:
            (at,) = struct.unpack_from(self.order + self._offset, self.data, at)
            if at + size > len(self.data):
                raise DirectoryError("outside", tag=tag, at=at)
        return at

    def ints(self, tag, types):
        """the entry's integers as a tuple, None when the tag is absent; ``types``: the allowed ones of BYTE, SHORT, LONG, LONG8"""
        if tag not in self.entries:
            return None
        typ, cnt, at = self.entries[tag]
        if typ not in types or cnt < 1:
            raise DirectoryError("type", tag=tag, type=typ, count=cnt)
        if TYPE_SIZE[typ] * cnt > self.inline:
            at = self._values_at(tag, TYPE_SIZE[typ] * cnt)
        return struct.unpack_from(f"{self.order}{cnt}{INT_FORMAT[typ]}", self.data, at)

    def raw_le(self, tag):
        """(type, one of TYPE_SIZE; count; value bytes in little-endian order: those of a big-endian file swapped per value)"""
        typ, cnt, _ = self.entries[tag]
        size, unit = TYPE_SIZE[typ] * cnt, UNIT_SIZE[typ]
        at = self._values_at(tag, size)
        raw = bytes(self.data[at:at + size])
        if self.order == ">" and unit > 1:
            raw = np.frombuffer(raw, dtype=f">u{unit}").astype(f"<u{unit}").tobytes()
        return typ, cnt, raw


def old_style_lzw(data, offsets, counts):
    """The index of the first of the LZW streams data[offset : offset + count] that is a pre-6.0, LSB-first one, None when there is
    none: libtiff recognises them by their first two bytes and decodes them its own way."""
    view = memoryview(data)
    return next((i for i, (o, c) in enumerate(zip(offsets, counts)) if c >= 2 and view[o] == 0 and view[o + 1] & 1), None)


def entry(tag, typ, values):
    """(tag, type, count, little-endian value bytes) of integer values, as ``build_ifd`` takes it"""
    return tag, typ, len(values), struct.pack(f"<{len(values)}{INT_FORMAT[typ]}", *values)


def ifd_size(n_entries, bigtiff) -> int:
    """the bytes of an IFD without its out-of-line values: entry count, entries, offset of the next IFD"""
    return (8 + 20 * n_entries + 8) if bigtiff else (2 + 12 * n_entries + 4)


def build_ifd(entries, ifd_offset, bigtiff, align=1) -> bytes:
    """The little-endian IFD of ``entries`` [(tag, type, count, value bytes)], written in the order given (TIFF wants ascending tags),
    as it must lie at ``ifd_offset``, with no next IFD.  Values that do not fit an entry follow the IFD in entry order, each at a
    multiple of ``align``."""
    wide, inline, limit = ("Q", 8, 1 << 64) if bigtiff else ("I", 4, 1 << 32)
    head = [struct.pack("<" + ("Q" if bigtiff else "H"), len(entries))]
    tail, at = [], ifd_offset + ifd_size(len(entries), bigtiff)
    for tag, typ, cnt, raw in entries:
        if len(raw) <= inline:
            value = raw.ljust(inline, b"\0")
        else:
            pad = -at % align
            tail.append(b"\0" * pad + raw)
            at += pad
            if at + len(raw) > limit:
                raise ValueError("a classic TIFF holds offsets below 2^32 only: use bigtiff=True")
            value = struct.pack("<" + wide, at)
            at += len(raw)
        head.append(struct.pack("<HH" + wide, tag, typ, cnt) + value)
    head.append(b"\0" * inline)
    return b"".join(head + tail)
