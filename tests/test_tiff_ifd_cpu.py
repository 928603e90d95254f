"""flair_amd/tiff_ifd.py, the one reader and the one builder of TIFF directories: the framers expressed through ``build_ifd`` produce the
bytes they produced before (tests/golden/tiff_framing.json), and ``Directory`` returns what was written, for classic TIFF and BigTIFF
in either byte order."""
import json
import os
import struct

import numpy as np
import pytest

import raster_reader_cases as rc
import raster_writer_cases as wc
import tiff_framing_cases as fc

CASES = fc.framing_inputs()


@pytest.fixture(scope="module")
def golden(golden_dir):
    with open(os.path.join(golden_dir, "tiff_framing.json")) as f:
        return json.load(f)


def test_the_golden_file_covers_the_cases(golden):
    assert set(golden) == set(CASES)
    names = [n for n in CASES if n.startswith("ifd_")]
    assert len(names) == 4 * 2 * 2 * 2 and {"lzw_file_1_strips", "lzw_file_4_strips"} <= set(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_framed_bytes_are_the_recorded_ones(golden, name):
    got = fc.frame(*CASES[name])
    want = bytes.fromhex(golden[name])
    assert got == want, f"{len(got)} bytes for {len(want)}, first difference at {next((i for i, (p, q) in enumerate(zip(got, want)) if p != q), None)}"


def test_lzw_file_keeps_its_arrays_behind_the_ifd():
    data = fc.frame(*CASES["lzw_file_4_strips"])
    t = wc.parse_ifd(data)
    assert struct.unpack_from("<I", data, 8 + 2 + 12 * t["order"].index(273) + 8)[0] == 134 and t[273][3][0] == 134 + 32
    one = wc.parse_ifd(fc.frame(*CASES["lzw_file_1_strips"]))
    assert one[273][3] == (134,) and one[279][3] == (20,)


# ---------------------------------------------------------------------------------------------------------- parse after build
UNIT = {1: 1, 2: 1, 3: 2, 4: 4, 5: 4, 12: 8, 16: 8}    # bytes swapped as one: a RATIONAL is two LONGs


def _swap_units(raw, unit):
    return b"".join(raw[i:i + unit][::-1] for i in range(0, len(raw), unit))


def _swap_to_mm(data: bytes, bigtiff: bool) -> bytes:
    """a little-endian file of a header and one IFD rewritten big-endian by hand, every value where it was"""
    cfmt, efmt, esize, inline, ofmt, hdr = ("Q", "HHQ", 20, 8, "Q", "2sHHHQ") if bigtiff else ("H", "HHI", 12, 4, "I", "2sHI")
    head = struct.unpack_from("<" + hdr, data, 0)
    out = bytearray(data)
    struct.pack_into(">" + hdr, out, 0, b"MM", *head[1:])
    ifd = head[-1]
    (n,) = struct.unpack_from("<" + cfmt, data, ifd)
    struct.pack_into(">" + cfmt, out, ifd, n)
    for i in range(n):
        at = ifd + struct.calcsize(cfmt) + esize * i
        tag, typ, cnt = struct.unpack_from("<" + efmt, data, at)
        struct.pack_into(">" + efmt, out, at, tag, typ, cnt)
        size, value = wc.TYPE_SIZE[typ] * cnt, at + esize - inline
        if size > inline:
            (where,) = struct.unpack_from("<" + ofmt, data, value)
            struct.pack_into(">" + ofmt, out, value, where)
            value = where
        out[value:value + size] = _swap_units(data[value:value + size], UNIT[typ])
    return bytes(out)


def _written(bigtiff):
    """the entries of the round trip: inline values, out-of-line arrays, a RATIONAL (out of line in a classic file, inline in a
    BigTIFF), DOUBLEs and ASCII"""
    from flair_amd.tiff_ifd import LONG, LONG8, SHORT, entry
    ints = [entry(256, LONG, [53]), entry(257, SHORT, [37]), entry(258, SHORT, [8, 8, 8, 8, 8]), entry(277, SHORT, [5]),
            entry(324, LONG8 if bigtiff else LONG, [16 + 48 * i for i in range(12)]), entry(325, LONG, [40 + i for i in range(12)])]
    raws = [(282, 5, 1, struct.pack("<2I", 300, 7)), (33550, 12, 3, struct.pack("<3d", 0.2, 0.2, 0.0)), (34737, 2, 6, b"RGF93\0")]
    return ints, raws


@pytest.mark.parametrize("order", ["<", ">"])
@pytest.mark.parametrize("bigtiff", [False, True])
def test_directory_returns_what_build_ifd_wrote(bigtiff, order):
    from flair_amd.raster_writer import tiled_tiff_header
    from flair_amd.tiff_ifd import INT_FORMAT, TYPE_SIZE, Directory, DirectoryError, build_ifd
    ints, raws = _written(bigtiff)
    entries = sorted(ints + raws)
    data = tiled_tiff_header(24, bigtiff).ljust(24, b"\xee") + build_ifd(entries, 24, bigtiff, align=8)
    if order == ">":
        data = _swap_to_mm(data, bigtiff)
    for view in (data, memoryview(data), np.frombuffer(data, np.uint8)):
        d = Directory(view)
        assert (d.order, d.bigtiff, d.ifd, d.count) == (order, bigtiff, 24, len(entries))
        assert list(d.entries) == [e[0] for e in entries]
        assert {tag: (typ, cnt) for tag, (typ, cnt, _) in d.entries.items()} == {tag: (typ, cnt) for tag, typ, cnt, _ in entries}
        for tag, typ, cnt, raw in entries:
            assert d.raw_le(tag) == (typ, cnt, raw), tag
        for tag, typ, cnt, raw in ints:
            assert d.ints(tag, INT_FORMAT) == struct.unpack(f"<{cnt}{INT_FORMAT[typ]}", raw)
    inline = 8 if bigtiff else 4
    assert {tag for tag, typ, cnt, _ in entries if TYPE_SIZE[typ] * cnt <= inline} == ({256, 257, 277, 282, 34737} if bigtiff else {256, 257, 277})
    assert d.ints(999, INT_FORMAT) is None
    with pytest.raises(DirectoryError) as e:
        d.ints(324, (3,))
    assert e.value.what == "type"
    with pytest.raises(DirectoryError) as e:
        Directory(data[:-1]).raw_le(34737 if not bigtiff else 33550)    # the last out-of-line value is cut
    assert e.value.what == "outside"
    for cut, what in ((6, "order"), (24 + 1, "ifd"), (24 + 30, "entries")):
        with pytest.raises(DirectoryError) as e:
            Directory(data[:cut])
        assert e.value.what == what


@pytest.mark.parametrize("order", ["<", ">"])
@pytest.mark.parametrize("bigtiff", [False, True])
def test_directory_reads_a_file_framed_by_hand(bigtiff, order):
    """the same four kinds from the framer of the raster reader's cases, which shares no code with tiff_ifd"""
    from flair_amd.tiff_ifd import INT_FORMAT, TAG, Directory
    raster = wc.labels(5, 37, 53, seed=33)
    data = rc.build_tiff(raster, tile=(16, 16), planar=2, bigtiff=bigtiff, order=order)
    d = Directory(data)
    assert (d.order, d.bigtiff) == (order, bigtiff)
    assert d.ints(TAG.ImageWidth, INT_FORMAT) == (53,) and d.ints(TAG.BitsPerSample, INT_FORMAT) == (8,) * 5
    offsets, counts = d.ints(TAG.TileOffsets, INT_FORMAT), d.ints(TAG.TileByteCounts, INT_FORMAT)
    assert len(offsets) == 60 and offsets[0] == (16 if bigtiff else 8) and d.ifd >= offsets[-1] + counts[-1]
    assert all(b == a + c + c % 2 for a, b, c in zip(offsets, offsets[1:], counts))


def test_old_style_lzw_is_told_by_two_bytes():
    from flair_amd.tiff_ifd import old_style_lzw
    data = b"\x00\x01rest" + b"\x80\x00" + b"\x00\x02" + b"\x00\xff"
    assert old_style_lzw(data, [0], [6]) == 0 and old_style_lzw(data, [6, 8, 10], [2, 2, 2]) == 2
    assert old_style_lzw(data, [6, 8], [2, 2]) is None and old_style_lzw(data, [0, 10], [1, 1]) is None
    assert old_style_lzw(memoryview(data), [10], [2]) == 0 and old_style_lzw(np.frombuffer(data, np.uint8), [10], [2]) == 0


def test_one_table_of_types_and_tags():
    from flair_amd import raster_reader, raster_writer, tiff_ifd
    assert raster_reader.TAG_NAMES is tiff_ifd.TAG_NAMES and tiff_ifd.TAG.TileOffsets == 324
    assert raster_writer.stream_groups is raster_reader.stream_groups and raster_writer.GROUP_BYTES == raster_reader.GROUP_BYTES
    assert raster_writer._staging is not raster_reader._staging
