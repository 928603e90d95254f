"""CPU side of the zone_detect raster writer (no device needed): ``raster_writer.tiled_tiff_header`` / ``tiled_tiff_ifd`` around streams of
the reference encoder give files that parse back to the raster and that PIL / libtiff read where they can read such files at all,
``read_geo_tags`` lifts the GeoTIFF tags of a source file as they are, and the helper's own tile streams equal a per-byte construction."""
import struct

import numpy as np
import pytest

import raster_writer_cases as rc


def _file(raster, tile, interleave, bigtiff, geo_tags=None):
    bands, H, W = raster.shape
    return rc.frame(H, W, bands, tile, interleave, rc.ref_streams(raster, tile, interleave), bigtiff=bigtiff, geo_tags=geo_tags)


@pytest.mark.parametrize("bigtiff", [True, False], ids=["bigtiff", "classic"])
@pytest.mark.parametrize("interleave", ["band", "pixel"])
@pytest.mark.parametrize("bands", [1, 2, 3, 13])
@pytest.mark.parametrize("shape", [(40, 56), (37, 53)], ids=["40x56", "37x53"])
def test_framed_files_read_back(shape, bands, interleave, bigtiff):
    raster = rc.labels(bands, *shape, seed=bands)
    data = _file(raster, 16, interleave, bigtiff)
    assert np.array_equal(rc.read_file(data), raster)
    t = rc.parse_ifd(data)
    assert t["bigtiff"] == bigtiff
    tags = t["order"]
    assert tags == sorted(tags) and len(set(tags)) == len(tags)
    assert set(tags) == {256, 257, 258, 259, 262, 277, 284, 322, 323, 324, 325, 339} | ({338} if bands in (2, 13) else set())
    assert t[284][3] == (2 if interleave == "band" and bands > 1 else 1,)
    ifd = struct.unpack_from("<Q" if bigtiff else "<I", data, 8 if bigtiff else 4)[0]
    for off, cnt in zip(t[324][3], t[325][3]):
        assert off % 16 == 0 and 16 <= off and off + cnt <= ifd   # the streams lie between the header and the IFD
    # PIL / libtiff where they read the layout: one band as L, three as RGB, two chunky bands once ExtraSamples says alpha
    if bands == 1:
        assert rc.pil_read(data)[0] == "L" and np.array_equal(rc.pil_read(data)[1], raster)
    elif bands == 3:
        mode, px = rc.pil_read(data)
        assert mode == "RGB" and np.array_equal(px, raster)
    elif bands == 2 and interleave == "pixel":
        mode, px = rc.pil_read(rc.patch_extra_samples(data))
        assert mode == "LA" and np.array_equal(px, raster)


def test_header():
    from flair_amd.raster_writer import tiled_tiff_header
    assert tiled_tiff_header(4096) == b"II\x2b\0\x08\0\0\0" + struct.pack("<Q", 4096)
    assert tiled_tiff_header(1 << 40, bigtiff=True)[8:] == struct.pack("<Q", 1 << 40)
    assert tiled_tiff_header(4096, bigtiff=False) == b"II\x2a\0" + struct.pack("<I", 4096)
    with pytest.raises(ValueError):
        tiled_tiff_header(1 << 32, bigtiff=False)


def test_classic_refuses_what_it_cannot_address():
    from flair_amd.raster_writer import tiled_tiff_ifd
    counts = [1 << 30] * 6     # a 32 x 48 raster at T = 16: six tiles of 1 GiB sum past 2^32
    offsets = [16 + i * (1 << 30) for i in range(6)]
    end = offsets[-1] + counts[-1]
    with pytest.raises(ValueError):
        tiled_tiff_ifd(32, 48, 1, 16, "band", offsets, counts, end, bigtiff=False)
    with pytest.raises(ValueError):   # the streams fit, the IFD's own arrays do not
        tiled_tiff_ifd(32, 48, 1, 16, "band", offsets[:3] + offsets[:3], counts, (1 << 32) - 64, bigtiff=False)
    assert tiled_tiff_ifd(32, 48, 1, 16, "band", offsets, counts, end, bigtiff=True)
    # the BigTIFF IFD of the same tiles, placed at 16 so that it can be parsed without 6 GiB in front of it: LONG8 arrays
    ifd = tiled_tiff_ifd(32, 48, 1, 16, "band", offsets, counts, 16, bigtiff=True)
    t = rc.parse_ifd(b"II\x2b\0\x08\0\0\0" + struct.pack("<Q", 16) + ifd)
    assert t[324][3] == tuple(offsets) and t[325][3] == tuple(counts) and t[324][0] == 16


def test_argument_errors():
    from flair_amd.raster_writer import tiled_tiff_ifd
    raster = rc.labels(1, 48, 48)
    streams = rc.ref_streams(raster, 16, "band")
    with pytest.raises(ValueError):
        rc.frame(48, 48, 1, 24, "band", streams[:4])          # tile = 24: no multiple of 16
    with pytest.raises(ValueError):
        rc.frame(48, 48, 1, 16, "band", streams[:8])          # 8 streams for 9 tiles
    with pytest.raises(ValueError):
        rc.frame(48, 48, 1, 16, "planar", streams)
    with pytest.raises(ValueError):
        tiled_tiff_ifd(48, 48, 1, 16, "band", [16] * 9, [4] * 9, 1024, geo_tags={33550: (12, 3, b"\0" * 23)})   # 3 doubles are 24 bytes
    with pytest.raises(ValueError):
        tiled_tiff_ifd(48, 48, 1, 16, "band", [16] * 9, [4] * 9, 1024, geo_tags={305: (2, 4, b"abc\0")})        # no GeoTIFF tag


@pytest.mark.parametrize("kind", ["classic_II", "classic_MM", "bigtiff_II", "bigtiff_MM"])
def test_geo_tags_round_trip(tmp_path, kind):
    from flair_amd.raster_writer import read_geo_tags
    src, want = rc.geo_source(bigtiff=kind.startswith("bigtiff"), order="<" if kind.endswith("II") else ">")
    path = tmp_path / "source.tif"
    path.write_bytes(src)
    tags = read_geo_tags(path)
    assert tags == want and sorted(tags) == [33550, 33922, 34735, 34737]
    if kind == "classic_II":
        from PIL import Image
        im = Image.open(path)                                   # the hand-framed source is a file libtiff reads
        assert np.asarray(im).tolist() == [[1, 2], [3, 4]] and im.tag_v2[34737] == "RGF93 / Lambert-93|"
        assert im.tag_v2[33550] == (0.2, 0.2, 0.0)
    raster = rc.labels(2, 40, 56)
    for bigtiff in (True, False):
        data = _file(raster, 16, "band", bigtiff, geo_tags=tags)
        t = rc.parse_ifd(data)
        assert t["order"] == sorted(t["order"])
        for tag, (typ, cnt, raw) in want.items():
            assert t[tag][:3] == (typ, cnt, raw), tag
        assert np.array_equal(rc.read_file(data), raster)
    single = _file(raster[:1], 16, "band", False, geo_tags=tags)   # PIL sees the tags of an output it can open
    from PIL import Image
    import io
    im = Image.open(io.BytesIO(single))
    assert im.tag_v2[33922] == (0.0, 0.0, 0.0, 880000.0, 6520000.0, 0.0) and im.tag_v2[34735] == struct.unpack("<16H", want[34735][2])


def test_geo_tags_of_plain_files_and_foreign_bytes(tmp_path):
    from flair_amd.raster_writer import read_geo_tags
    plain = tmp_path / "plain.tif"
    plain.write_bytes(_file(rc.labels(1, 40, 56), 16, "band", True))
    assert read_geo_tags(plain) == {}
    plain.write_bytes(_file(rc.labels(1, 40, 56), 16, "band", False))
    assert read_geo_tags(plain) == {}
    for i, junk in enumerate((b"", b"II", b"\x89PNG\r\n\x1a\n" + b"\0" * 64, b"II\x2c\0" + b"\0" * 32, b"II\x2a\0\xff\xff\xff\x7f")):
        p = tmp_path / f"junk{i}"
        p.write_bytes(junk)
        with pytest.raises(ValueError):
            read_geo_tags(p)


def test_restated_streams_equal_the_per_byte_construction():
    raster = rc.labels(3, 21, 37, seed=2)
    assert rc.tile_streams(raster, 16, "pixel") == rc.tile_streams_slow(raster, 16)
    f32 = rc.argmax_raster(20, 24)
    assert rc.tile_streams(f32, 16, "pixel", rc.ARGMAX_SCALE) == rc.tile_streams_slow(f32, 16, rc.ARGMAX_SCALE)
    # and band interleave is the same tiles, one band at a time
    band = rc.tile_streams(raster, 16, "band")
    assert len(band) == 3 * 2 * 3 and band[4] == rc.tile_streams(raster[:1], 16, "pixel")[4]
    assert band[6 + 5] == rc.tile_streams(raster[1:2], 16, "pixel")[5]


def test_fp32_conversion_restated():
    v = np.array([0.0, 1.0, 0.5, np.nextafter(np.float32(1), np.float32(0)), -0.1, 1.5, np.nan, 254.5 / 255, 1 / 255], np.float32)
    got = rc.to_bytes(np.stack([v, v]).reshape(2, 1, -1), (1.0, 255.0))
    assert got[0, 0].tolist() == [0, 1, 0, 0, 0, 1, 0, 0, 0]
    assert got[1, 0].tolist() == [0, 255, 127, 254, 0, 255, 0, 254, 1]


def test_stream_groups_cover_the_streams_once():
    from flair_amd.raster_writer import stream_groups
    assert stream_groups(12, 4, 256, 1 << 20) == [(0, 12)]
    assert stream_groups(12, 4, 256, 256 * 9) == [(0, 8), (8, 4)]       # whole tile rows
    assert stream_groups(12, 4, 256, 256 * 3) == [(0, 3), (3, 3), (6, 3), (9, 3)]
    assert stream_groups(3, 4, 256, 1) == [(0, 1), (1, 1), (2, 1)]      # one stream at least


def test_wrappers_refuse_host_tensors_and_bad_arguments(tmp_path):
    import torch
    from flair_amd import ops, raster_writer
    from flair_amd._lib import FlairHipError
    u8 = torch.zeros(2, 32, 32, dtype=torch.uint8)
    with pytest.raises(FlairHipError):
        ops.tiff_lzw_encode_tiles(u8, 16)
    with pytest.raises(ValueError):
        ops.tiff_lzw_encode_tiles(u8, 24)
    with pytest.raises(ValueError):
        ops.tiff_lzw_encode_tiles(u8, 16, interleave="planar")
    with pytest.raises(ValueError):
        ops.tiff_lzw_encode_tiles(u8, 16, scale=(1.0, 255.0))      # bytes take no scale
    with pytest.raises(ValueError):
        ops.tiff_lzw_encode_tiles(u8.float(), 16)                   # fp32 needs one
    with pytest.raises(ValueError):
        ops.tiff_tile_streams(2, 32, 32, 16, "planar")
    with pytest.raises(FlairHipError):
        ops.tiff_lzw_encode_tiles(u8.to(torch.int32), 16)
    with pytest.raises(ValueError):
        ops.tiff_pack_streams(torch.zeros(0, 64, dtype=torch.uint8), torch.zeros(0, dtype=torch.int32), 64)
    with pytest.raises(FlairHipError):
        ops.tiff_pack_streams(torch.zeros(2, 64, dtype=torch.uint8), torch.zeros(2, dtype=torch.int32), 64)
    assert ops.tiff_lzw_tile_slot_bytes(16, 1) == ops.tiff_lzw_slot_bytes(1, 256)
    assert ops.tiff_lzw_tile_slot_bytes(512, 13) == ops.tiff_lzw_slot_bytes(1, 512 * 512 * 13)
    assert ops.tiff_lzw_tile_slot_bytes(0, 1) < 0 and ops.tiff_lzw_tile_slot_bytes(16, 0) < 0
    assert ops.tiff_tile_streams(13, 40, 56, 16, "band") == 13 * 3 * 4 and ops.tiff_tile_streams(13, 40, 56, 16, "pixel") == 12
    with pytest.raises(RuntimeError):
        raster_writer.write_raster(tmp_path / "x.tif", u8, 16)      # a host tensor
    assert not (tmp_path / "x.tif").exists()
    import flair_amd
    assert flair_amd.write_raster is raster_writer.write_raster and flair_amd.read_geo_tags is raster_writer.read_geo_tags
    assert flair_amd.tiled_tiff_ifd is raster_writer.tiled_tiff_ifd and flair_amd.tiled_tiff_header is raster_writer.tiled_tiff_header
