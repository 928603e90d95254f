"""CPU suite of the raster reader (flair_amd/raster_reader.py, csrc/tiff_read.hip): which files raster_layout accepts and what it says
about those it refuses, the cases the GPU tests decode (their sources must lie on every side of the decoder's window and flush
block), the two contracts of flair_tiff_chunks_to_planes restated in numpy, and the declarations of the new symbols."""
import os
import re

import numpy as np
import pytest

import raster_reader_cases as rc
import raster_writer_cases as wc
import tiff_lzw_cases as tc
import tiff_lzw_decode_cases as dc
from flair_amd import raster_reader as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW = rr.CHUNK_WINDOW


@pytest.mark.parametrize("name", sorted(rc.accepted_files()))
def test_layout_of_accepted_files(name):
    data, want = rc.accepted_files()[name]
    lay = rr.raster_layout(data)
    assert (lay.bands, lay.H, lay.W) == want.shape
    assert lay.n_chunks == len(lay.offsets) == len(lay.counts) and lay.order == ("<" if data[:2] == b"II" else ">")
    assert lay.bigtiff == (data[2:4] in (b"\x2b\x00", b"\x00\x2b"))
    table = lay.chunk_table()
    assert table.shape == (lay.n_chunks, 5) and table.dtype == np.int32
    # the reference decoder through the layout alone gives the pixels: what read_raster must return on the device
    slots = []
    for (x0, y0, width, rows, band0), off, cnt in zip(table, lay.offsets, lay.counts):
        raw = bytes(data[off:off + cnt])
        want_len = int(width) * int(rows) * lay.samples
        px, status = (raw[:want_len], 0) if lay.compression == 1 else dc.lzw_decode_strip(raw, want_len)
        assert status == 0 and len(px) == want_len
        slots.append(px)
    got = rc.planes_ref(slots, table, [0] * len(slots), lay.samples, lay.predictor, np.full(want.shape, rc.FILL, np.uint8))
    assert np.array_equal(got, want)


def test_layout_fields_of_the_families():
    f = rc.accepted_files()
    lay = rr.raster_layout(f["framed_band_big"][0])
    assert (lay.tiled, lay.planar, lay.chunk_w, lay.chunk_h, lay.compression, lay.predictor, lay.n_chunks) == (True, 2, 16, 16, 5, 1, 60)
    lay = rr.raster_layout(f["framed_pixel_classic"][0])
    assert (lay.planar, lay.samples, lay.n_chunks, lay.bigtiff) == (1, 5, 12, False)
    lay = rr.raster_layout(f["pil_RGB_pred2"][0])
    assert (lay.tiled, lay.planar, lay.bands, lay.predictor, lay.chunk_w) == (False, 1, 3, 2, 45)
    assert rr.raster_layout(f["pil_L"][0]).predictor == 1
    lay = rr.raster_layout(f["strips_band_pred2"][0])
    assert (lay.tiled, lay.planar, lay.chunk_h, lay.n_chunks) == (False, 2, 7, 5 * 6)
    assert [tuple(r) for r in lay.chunk_table()[[0, 5, 6]]] == [(0, 0, 53, 7, 0), (0, 35, 53, 2, 0), (0, 0, 53, 7, 1)]
    lay = rr.raster_layout(f["tiles_16x32_pixel_pred2"][0])
    assert (lay.chunk_w, lay.chunk_h, lay.chunks_x, lay.chunks_y) == (16, 32, 4, 2)
    assert "tile at row 32, column 16" in lay.chunk_name(5)
    assert rr.raster_layout(memoryview(f["mm_classic_tiled"][0])).order == ">"


def test_pil_writes_the_predictor():
    """the PIL-written predictor-2 strips decode to the image only after the running sum"""
    data, want = rc.accepted_files()["pil_RGB_pred2"]
    lay = rr.raster_layout(data)
    rows = int(lay.chunk_table()[0][3])
    px, status = dc.lzw_decode_strip(bytes(data[lay.offsets[0]:lay.offsets[0] + lay.counts[0]]), rows * lay.W * 3)
    raw = np.frombuffer(px, np.uint8).reshape(rows, lay.W * 3)
    top = want[:, :rows].transpose(1, 2, 0).reshape(rows, -1)
    assert status == 0 and not np.array_equal(raw, top) and np.array_equal(rc.unpredict(raw, 3), top)


@pytest.mark.parametrize("name", sorted(rc.refused_files()))
def test_refusals_name_the_tag(name):
    data, word = rc.refused_files()[name]
    with pytest.raises(rr.UnsupportedRaster) as e:
        rr.raster_layout(data)
    assert word in str(e.value), str(e.value)
    assert isinstance(e.value, ValueError)


def test_refusals_say_the_value():
    f = rc.refused_files()
    for name, text in (("deflate", "Compression (259) is 8"), ("bits_16", "[16, 16]"), ("tile_width_24", "TileWidth (322) is 24"),
                       ("offsets_too_few", "holds 23 values"), ("lsb_first_lzw", "chunk 3")):
        with pytest.raises(rr.UnsupportedRaster, match=re.escape(text)):
            rr.raster_layout(f[name][0])


def test_read_plan_groups_and_reads():
    data, _ = rc.accepted_files()["framed_band_big"]
    lay = rr.raster_layout(data)
    groups, slot, src_off, reads = rr.read_plan(lay, group_bytes=3000)
    assert slot == 256 and groups[0] == (0, 8) and sum(n for _, n in groups) == 60 and len(reads) == len(groups)
    for (first, n), (nbytes, runs) in zip(groups, reads):
        buf = bytearray(nbytes)
        for file_off, length, at in runs:
            buf[at:at + length] = data[file_off:file_off + length]
        for i in range(first, first + n):      # every chunk's bytes lie where src_off says
            assert bytes(buf[src_off[i]:src_off[i] + lay.counts[i]]) == data[lay.offsets[i]:lay.offsets[i] + lay.counts[i]]
    assert len(rr.read_plan(lay)[0]) == 1
    # chunks far apart in the file are read by themselves, in file order, whatever the order of the offset array
    far = rr.RasterLayout(**{**lay.__dict__, "offsets": lay.offsets[::-1] * 100000, "counts": lay.counts})
    _, _, off2, reads2 = rr.read_plan(far)
    assert len(reads2[0][1]) == 60 and reads2[0][0] < 2 * int(lay.counts.sum()) + 16 * 60 and off2[59] == 0


# ------------------------------------------------------------------------------------------------ the decoder's cases
@pytest.mark.parametrize("name", sorted(rc.window_streams(WINDOW)))
def test_position_decode_is_the_reference_decode(name):
    """the tracer that classifies the cases decodes what the reference decodes, and the kernel's ring / flush / read-back rules,
    replayed on the host, never read a ring place that was overwritten or a slot byte that is not flushed"""
    stream, raw, (px, status) = rc.window_chunks(WINDOW)[name]
    assert status == 0 and px == raw
    for window in (None, WINDOW):
        got, st, _ = rc.trace_decode(stream, len(raw), window)
        assert st == 0 and got == raw


def test_cases_lie_on_every_side_of_the_window_and_the_block():
    counts = {name: rc.boundary_counts(rc.trace_decode(s, len(raw))[2], WINDOW) for name, (s, raw, _) in rc.window_chunks(WINDOW).items()}
    far = counts["far_80000"]
    assert far["far"] >= 100 and far["back"] >= far["far"] and far["ring"] > 0 and far["longest"] > 300
    for side in ("back", "ring", "across", "flushed", "unflushed", "half"):
        assert sum(c[side] for c in counts.values()) > 0, side
    assert counts["edge_+1"]["across"] > 50 and counts["edge_+0"]["across"] == 0 and counts["edge_-1"]["back"] == 0
    assert counts["edge_+2"]["back"] > 50
    long_across = [n for op, frm, n in rc.trace_decode(*rc.window_chunks(WINDOW)["long_across"][:1], len(rc.window_streams(WINDOW)["long_across"]))[2]
                   if frm < op - WINDOW < frm + n]
    assert long_across and max(long_across) > 64      # a source across the window that takes more than one 64-byte step
    assert counts["far_repeat"]["back"] > 300         # read-backs in three places, new output in between


def test_malformed_cases_have_their_status():
    m = rc.malformed_chunks()
    want = {"truncated": 1, "truncated_far": 1, "empty": 1, "eoi_first": 2, "eoi_early": 2, "table_code_after_clear": 3,
            "table_code_first": 3, "code_above_next": 4, "no_eoi_needed": 0, "stored_short": 1, "stored_long": 0}
    assert set(m) == set(want)
    for name, (stream, n, mode) in m.items():
        px, status = rc.reference_chunk(stream, n, mode)
        assert status == want[name], name
        if mode == 1:
            got, st, _ = rc.trace_decode(stream, n, WINDOW)
            assert (got, st) == (px, status), name
    assert len(rc.reference_chunk(*m["truncated"])[0]) > WINDOW and len(rc.reference_chunk(*m["eoi_early"])[0]) == 450


def test_chunk_launch_offsets_take_every_alignment():
    chunks = [(bytes([i]) * (5 + i), 10, 0) for i in range(8)]
    src, off, ln, dn, md, slot = rc.chunk_launch(chunks, misalign=1)
    assert {int(o) % 4 for o in off} == {0, 1, 2, 3} and slot == 128
    for i, (s, _, _) in enumerate(chunks):
        assert src[off[i]:off[i] + ln[i]].tobytes() == s


# ------------------------------------------------------------------------------------------------ chunks_to_planes, restated
def test_predictor_2_is_the_running_sum_per_sample():
    tile = np.random.default_rng(4).integers(0, 256, (16, 16 * 3)).astype(np.uint8)
    assert np.array_equal(rc.unpredict(tile, 3), rc.unpredict_slow(tile, 3))
    assert np.array_equal(rc.unpredict(rc.predict(tile, 3), 3), tile) and np.array_equal(rc.unpredict(tile, 1), rc.unpredict_slow(tile, 1))
    assert rc.unpredict(np.full((1, 600), 1, np.uint8), 1)[0, -1] == 600 % 256     # modulo 256, over more than one 64-pixel trip


def test_clipping_and_skipping_restated():
    raster = wc.labels(3, 37, 53, seed=2)
    for planar, tiled, cw, ch in ((1, True, 16, 16), (2, True, 16, 32), (2, False, 53, 7)):
        table = rc.chunk_grid(37, 53, 3, planar, cw, ch, tiled)
        slots = [rc.chunk_bytes(raster, planar, *row).tobytes() for row in table]
        status = [0] * len(table)
        got = rc.planes_ref(slots, table, status, 3 if planar == 1 else 1, 1, np.full((3, 37, 53), rc.FILL, np.uint8))
        assert np.array_equal(got, raster)
        status[1] = 4
        got = rc.planes_ref(slots, table, status, 3 if planar == 1 else 1, 1, np.full((3, 37, 53), rc.FILL, np.uint8))
        x0, y0, width, rows, band0 = table[1]
        hole = got[band0:band0 + (3 if planar == 1 else 1), y0:y0 + rows, x0:x0 + width]
        assert (hole == rc.FILL).all() and (got != raster).sum() == (hole != raster[band0:band0 + hole.shape[0], y0:y0 + rows, x0:x0 + width]).sum()
    # byte by byte: pixel (r, x) of a chunk, sample k, is planes[band0 + k][y0 + r][x0 + x] when inside
    table = rc.chunk_grid(37, 53, 3, 1, 16, 16, True)
    for (x0, y0, width, rows, band0) in table[[0, 3, 11]]:
        chunk = rc.chunk_bytes(raster, 1, x0, y0, width, rows, band0).reshape(rows, width, 3)
        for r in range(rows):
            for x in range(width):
                inside = y0 + r < 37 and x0 + x < 53
                assert tuple(chunk[r, x]) == (tuple(raster[:, y0 + r, x0 + x]) if inside else (0, 0, 0))


# ------------------------------------------------------------------------------------------------ declarations
def test_new_symbols_are_declared_and_bound():
    import ctypes as C
    from flair_amd import _lib as L
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flair_hip.h")).read(), flags=re.S)
    kinds = {"int": C.c_int, "long": C.c_long}
    for name in ("flair_tiff_lzw_decode_chunks_cap", "flair_tiff_lzw_decode_chunks_window", "flair_tiff_lzw_decode_chunks",
                 "flair_tiff_chunks_to_planes"):
        m = re.search(r"\b(int|long)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{name} is not declared in include/flair_hip.h"
        res, args = L.PROTOTYPES[name]
        assert res is kinds[m.group(1)]
        params = [p.strip() for p in m.group(2).split(",")] if m.group(2).strip() != "void" else []
        assert len(params) == len(args), name
        for p, a in zip(params, args):
            want = C.c_void_p if "*" in p else kinds[p.split()[0]]
            assert a is want, (name, p)


def test_constants_and_exports():
    import flair_amd
    assert rr.CHUNK_CAP >= 8 << 20 and rr.CHUNK_WINDOW > rr.FLUSH_BLOCK == rc.BLOCK
    for name in ("read_raster", "raster_layout", "RasterLayout", "UnsupportedRaster", "RasterDecodeError", "raster_reader"):
        assert name in flair_amd.__all__ and hasattr(flair_amd, name)
    from flair_amd.zone_detect import ZoneDetector
    assert callable(ZoneDetector.read) and callable(ZoneDetector.run_files)
    assert issubclass(rr.RasterDecodeError, RuntimeError)
    assert tc.lzw_strip(b"ab")   # the helper the cases lean on
