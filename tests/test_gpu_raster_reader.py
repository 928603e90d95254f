"""tiff_lzw_decode_chunks_kernel and tiff_chunks_to_planes_kernel (csrc/tiff_read.hip) through flair_amd.ops, and
raster_reader.read_raster / ZoneDetector.read / run_files on top of them.  Everything is bit-exact: the decoder against the reference
decoder (bytes and status, guard bytes around every slot), the scatter against its numpy restatement, whole files against the pixels
their writer was given."""
import numpy as np
import pytest
import torch

import raster_reader_cases as rc
import raster_writer_cases as wc
import tiff_lzw_cases as tc
import tiff_lzw_decode_cases as dc
from flair_amd import raster_reader as rr

pytestmark = pytest.mark.gpu

WINDOW = rr.CHUNK_WINDOW


def _decode(dev, chunks, slot_bytes=None, misalign=0, src_off=None, src_bytes=None):
    """one launch over (stream, dst_len, mode) triples into 0xA5-filled slots with a guard slot before and after: (slots as numpy
    (n, slot), status, the whole buffer with its guard slots).  ``src_off`` replaces offsets, ``src_bytes`` cuts the source short (for
    the range errors)."""
    from flair_amd import ops
    src, off, ln, dn, md, slot = rc.chunk_launch(chunks, slot_bytes, misalign)
    if src_off is not None:
        off = np.array(src_off, np.int64)
    n = len(chunks)
    buf = torch.full(((n + 2) * slot,), rc.FILL, dtype=torch.uint8, device=dev)
    up = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    d_src = up(src if src_bytes is None else src[:src_bytes].copy())
    slots, status = ops.tiff_lzw_decode_chunks(d_src, up(off), up(ln), up(dn), up(md), slot, out=buf[slot:(n + 1) * slot])
    whole = buf.cpu().numpy().reshape(n + 2, slot)
    assert (whole[0] == rc.FILL).all() and (whole[-1] == rc.FILL).all()
    assert slots.data_ptr() == buf.data_ptr() + slot
    return whole[1:-1], status.cpu().numpy(), whole


def _check(chunks, slots, status, whole):
    """bytes and status of every chunk equal the reference's; every other byte of the buffer (the rest of a slot, the guard slots)
    still holds the fill"""
    written = []
    for i, (stream, n, mode) in enumerate(chunks):
        px, st = rc.reference_chunk(stream, n, mode)
        assert status[i] == st, (i, status[i], st)
        assert slots[i, :len(px)].tobytes() == px, i
        written.append(len(px))
    slot = whole.shape[1]
    assert dc.guards_intact(whole.reshape(-1), [(i + 1) * slot for i in range(len(chunks))], written, rc.FILL)


def test_window_constant_and_cap(dev):
    from flair_amd import ops
    assert ops.tiff_lzw_decode_chunks_window() == rr.CHUNK_WINDOW
    assert ops.tiff_lzw_decode_chunks_cap() == rr.CHUNK_CAP >= 8 << 20


def test_sources_on_every_side_of_the_window(dev):
    """the tracer cases: table codes copied from the ring, from the slot (more than 65 536 bytes back too) and from both"""
    cases = rc.window_chunks(WINDOW)
    chunks = [(s, len(raw), 1) for s, raw, _ in cases.values()]
    slots, status, whole = _decode(dev, chunks)
    for i, (name, (s, raw, (px, st))) in enumerate(cases.items()):
        assert st == 0 and px == raw and status[i] == 0, name
        assert slots[i, :len(raw)].tobytes() == raw, name
    _check(chunks, slots, status, whole)


def test_clears_in_mid_stream_and_a_full_table(dev):
    raw = dc.values_strip(30000, 200, seed=5)
    smooth = tc.smooth_mask().tobytes()[:100000]
    chunks = [(dc.lzw_strip_with_clears(raw, 700), len(raw), 1),
              (dc.lzw_strip_with_clears(raw, 10 ** 9, reset_at=None), len(raw), 1),      # the table fills up, 12-bit codes go on
              (dc.lzw_strip_with_clears(raw, 10 ** 9, reset_at=4094), len(raw), 1),
              (dc.lzw_strip_with_clears(smooth, 1500), len(smooth), 1),
              (tc.lzw_strip(smooth), len(smooth), 1)]
    for s, n, _ in chunks:
        assert dc.lzw_decode_strip(s, n)[1] == 0
    _check(chunks, *_decode(dev, chunks))


@pytest.mark.parametrize("misalign", [1, 2, 3])
def test_lengths_alignments_and_many_chunks(dev, misalign):
    chunks = [(tc.lzw_strip(raw), len(raw), 1) for raw in rc.length_streams(WINDOW).values()]
    chunks += [(tc.lzw_strip(dc.values_strip(n, 3 + n % 11, seed=n)), n, 1) for n in range(1000, 1040)]     # many, all different
    chunks += [(dc.values_strip(777, 256, seed=1), 777, 0), (dc.values_strip(4096, 256, seed=2), 4096, 0)]   # stored ones among them
    slots, status, whole = _decode(dev, chunks, misalign=misalign)
    assert (status == 0).all()
    _check(chunks, slots, status, whole)


def test_malformed_streams_have_defined_outcomes(dev):
    m = rc.malformed_chunks()
    chunks = list(m.values())
    slots, status, whole = _decode(dev, chunks)
    _check(chunks, slots, status, whole)
    assert dict(zip(m, status.tolist()))["code_above_next"] == 4


def test_range_and_cap_errors_write_nothing(dev):
    good = (tc.lzw_strip(b"abc" * 100), 300, 1)
    # dst_len below 1 and above the slot, a mode that is none, a negative length is impossible to frame: the offsets do it
    chunks = [good, (good[0], 0, 1), (good[0], 129 * 128, 1), (good[0], 300, 2), (good[0], 300, -1), good]
    slots, status, _ = _decode(dev, chunks, slot_bytes=128 * 128)
    assert status.tolist() == [0, 5, 5, 5, 5, 0]
    for i in (1, 2, 3, 4):
        assert (slots[i] == rc.FILL).all()
    assert slots[0, :300].tobytes() == slots[5, :300].tobytes() == b"abc" * 100
    # offsets outside the source: below 0, past the end, the last byte outside
    src_len = len(good[0])
    chunks = [good, good, good, good]
    total = len(rc.chunk_launch(chunks)[0])
    slots, status, _ = _decode(dev, chunks, src_off=[0, -1, total, total - src_len + 1])
    assert status.tolist() == [0, 5, 5, 5] and (slots[1:] == rc.FILL).all()
    # a decoded length above the cap, in a slot that could hold it; its neighbour decodes
    cap = rr.CHUNK_CAP
    slots, status, _ = _decode(dev, [good, (good[0], cap + 1, 1), (good[0], cap + 1, 0)], slot_bytes=cap + 128)
    assert status.tolist() == [0, 5, 1] and (slots[1] == rc.FILL).all()
    assert slots[2, :src_len].tobytes() == good[0] and (slots[2, src_len:] == rc.FILL).all()    # stored chunks have no cap


def test_argument_errors(dev):
    from flair_amd import _lib as L
    from flair_amd import ops
    lib = L.lib()
    src = torch.zeros(64, dtype=torch.uint8, device=dev)
    off = torch.zeros(1, dtype=torch.int64, device=dev)
    i32 = torch.ones(1, dtype=torch.int32, device=dev)
    buf = torch.zeros(1024, dtype=torch.uint8, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    call = lambda s, n, scratch, slot: lib.flair_tiff_lzw_decode_chunks(s, 64, L.ptr(off), L.ptr(i32), L.ptr(i32), L.ptr(i32), n, scratch,  # noqa: E731
                                                                       slot, L.ptr(st), L.stream())
    assert call(None, 1, L.ptr(buf), 128) == -1 and call(L.ptr(src), 0, L.ptr(buf), 128) == -1 and call(L.ptr(src), 1, L.ptr(buf), 0) == -1
    assert call(L.ptr(src), 1, L.ptr(buf[1:]), 128) == -2 and call(L.ptr(src), 1, L.ptr(buf), 100) == -2
    assert call(L.ptr(src), 1, L.ptr(buf), 128) == 0
    planes = torch.zeros(2, 4, 4, dtype=torch.uint8, device=dev)
    table = torch.zeros(1, 5, dtype=torch.int32, device=dev)
    to = lambda samples, pred, rows: lib.flair_tiff_chunks_to_planes(L.ptr(buf), 128, L.ptr(table), L.ptr(st), 1, rows, samples, pred,  # noqa: E731
                                                                     L.ptr(planes), 2, 4, 4, L.stream())
    assert to(3, 1, 1) == -1 and to(2, 3, 1) == -1 and to(2, 1, 0) == -1 and to(2, 2, 1) == 0 and to(1, 1, 1) == 0
    with pytest.raises(ValueError):
        ops.tiff_lzw_decode_chunks(src, off, i32, i32, i32, 100)
    with pytest.raises(L.FlairHipError):
        ops.tiff_lzw_decode_chunks(src, off.int(), i32, i32, i32, 128)
    with pytest.raises(ValueError):
        ops.tiff_chunks_to_planes(buf.view(8, 128), torch.zeros(8, 5, dtype=torch.int32, device=dev), torch.zeros(8, dtype=torch.int32, device=dev),
                                  planes, 3)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ chunks_to_planes
def _to_planes(dev, raster, planar, cw, ch, tiled, predictor, bad=()):
    """the kernel and the restatement on the chunks of ``raster``; chunks in ``bad`` carry status 4"""
    from flair_amd import ops
    bands, H, W = raster.shape
    samples = bands if planar == 1 else 1
    table = rc.chunk_grid(H, W, bands, planar, cw, ch, tiled)
    raw = []
    for row in table:
        chunk = rc.chunk_bytes(raster, planar, *row)
        raw.append((rc.predict(chunk, samples) if predictor == 2 else chunk).tobytes())
    slot = -(-max(len(s) for s in raw) // 128) * 128
    scratch = np.full((len(raw), slot), 0x3C, np.uint8)
    for i, s in enumerate(raw):
        scratch[i, :len(s)] = np.frombuffer(s, np.uint8)
    status = np.zeros(len(raw), np.int32)
    status[list(bad)] = 4
    planes = torch.full((bands, H, W), rc.FILL, dtype=torch.uint8, device=dev)
    got = ops.tiff_chunks_to_planes(torch.from_numpy(scratch).to(dev), torch.from_numpy(table).to(dev), torch.from_numpy(status).to(dev),
                                    planes, samples, predictor)
    assert got is planes
    want = rc.planes_ref(raw, table, status, samples, predictor, np.full((bands, H, W), rc.FILL, np.uint8))
    return planes.cpu().numpy(), want


@pytest.mark.parametrize("predictor", [1, 2])
@pytest.mark.parametrize("planar", [1, 2])
@pytest.mark.parametrize("bands", [1, 2, 3, 5])
def test_tiles_to_planes(dev, bands, planar, predictor):
    for (H, W), (cw, ch) in (((40, 56), (16, 16)), ((37, 53), (16, 16)), ((37, 53), (16, 32)), ((40, 56), (32, 16))):
        raster = wc.noise(bands, H, W, seed=bands + H)
        got, want = _to_planes(dev, raster, planar, cw, ch, True, predictor)
        assert np.array_equal(want, raster)           # the restatement inverts the framing: nothing of the fill is left
        assert np.array_equal(got, want), (H, W, cw, ch)


@pytest.mark.parametrize("predictor", [1, 2])
@pytest.mark.parametrize("planar", [1, 2])
def test_strips_to_planes(dev, planar, predictor):
    for bands, (H, W) in ((1, (37, 53)), (5, (37, 53)), (3, (20, 333))):       # 333 pixels: six trips of the scan and their carries
        raster = wc.noise(bands, H, W, seed=7 * bands)
        for rows in (1, 7, H):
            got, want = _to_planes(dev, raster, planar, W, rows, False, predictor)
            assert np.array_equal(want, raster) and np.array_equal(got, want), (bands, rows)


def test_a_wide_strip_row_carries_through_every_trip(dev):
    raster = np.ones((2, 3, 10240), np.uint8)
    raster[1] = wc.noise(1, 3, 10240, seed=3)[0]
    for planar in (1, 2):
        got, want = _to_planes(dev, raster, planar, 10240, 2, False, 2)
        assert np.array_equal(got, want) and np.array_equal(got, raster)


def test_failed_chunks_leave_their_rectangle(dev):
    raster = wc.noise(3, 40, 56, seed=4)
    for planar in (1, 2):
        got, want = _to_planes(dev, raster, planar, 16, 16, True, 2, bad=(1, 6))
        assert np.array_equal(got, want)
        x0, y0 = 16, 0                                # chunk 1
        assert (got[0, y0:y0 + 16, x0:x0 + 16] == rc.FILL).all() and (got != raster).any()


# ------------------------------------------------------------------------------------------------------------ read_raster
@pytest.mark.parametrize("name", sorted(rc.accepted_files()))
def test_read_raster_of_every_family(dev, tmp_path, name):
    data, want = rc.accepted_files()[name]
    (tmp_path / "r.tif").write_bytes(data)
    got = rr.read_raster(tmp_path / "r.tif", dev)
    assert got.dtype == torch.uint8 and got.device.type == "cuda" and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), want)
    small = rr.read_raster(tmp_path / "r.tif", dev, group_bytes=1)      # one chunk a group
    assert torch.equal(small, got)


@pytest.mark.parametrize("interleave", ["band", "pixel"])
def test_write_then_read_is_the_identity(dev, tmp_path, interleave):
    from flair_amd.raster_writer import write_raster
    raster = np.concatenate([wc.smooth_blobs(520, 530), wc.noise(2, 520, 530), wc.labels(2, 520, 530)])
    x = torch.from_numpy(raster).to(dev)
    info = write_raster(tmp_path / "w.tif", x, 256, interleave=interleave)
    assert torch.equal(rr.read_raster(tmp_path / "w.tif", dev), x)
    lay = rr.raster_layout((tmp_path / "w.tif").read_bytes())
    assert lay.n_chunks == info["streams"] and (lay.chunk_w, lay.chunk_h, lay.bands) == (256, 256, 5)
    three = -(-lay.n_chunks // 3) * 256 * 256 * lay.samples
    assert len(rr.read_plan(lay, three)[0]) == 3
    assert torch.equal(rr.read_raster(tmp_path / "w.tif", dev, group_bytes=three), x)


def test_a_corrupted_tile_is_named(dev, tmp_path):
    raster = wc.labels(5, 40, 56, seed=31)
    streams = wc.ref_streams(raster, 16, "band")
    streams[17] = streams[17][:len(streams[17]) // 2]                      # the bytes run out: status 1
    (tmp_path / "cut.tif").write_bytes(wc.frame(40, 56, 5, 16, "band", streams))
    with pytest.raises(rr.RasterDecodeError, match=r"chunk 17 \(tile at row 16, column 16, band 1\).*status 1") as e:
        rr.read_raster(tmp_path / "cut.tif", dev)
    assert (e.value.chunk, e.value.status) == (17, 1)
    streams[17] = dc.pack_codes([(256, 9), (65, 9), (400, 9)])             # a code the table does not hold: status 4
    (tmp_path / "bad.tif").write_bytes(wc.frame(40, 56, 5, 16, "band", streams))
    with pytest.raises(rr.RasterDecodeError, match="status 4"):
        rr.read_raster(tmp_path / "bad.tif", dev, group_bytes=1)
    with pytest.raises(rr.UnsupportedRaster, match="Compression"):
        (tmp_path / "deflate.tif").write_bytes(rc.refused_files()["deflate"][0])
        rr.read_raster(tmp_path / "deflate.tif", dev)
    with pytest.raises(RuntimeError):
        rr.read_raster(tmp_path / "cut.tif", "cpu")


# ------------------------------------------------------------------------------------------------------------ ZoneDetector
def test_zone_detector_from_file_to_file(dev, tmp_path):
    import flair_amd
    from flair_amd.zone_detect import ZoneDetector
    C = 13
    torch.manual_seed(5)
    model = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=C, compute_dtype="f32").to(dev).eval()
    cfg = {"img_pixels_detection": 64, "margin": 16, "output_type": "argmax", "n_classes": C, "batch_size": 4, "channels": [1, 2, 3, 4, 5],
           "norma_task": [{"norm_type": "scaling"}], "classes": {i + 1: [1.0, f"c{i}"] for i in range(C)}}
    raster = wc.noise(5, 96, 112, seed=12)
    _, geo = wc.geo_source()
    src, dst = tmp_path / "src.tif", tmp_path / "dst.tif"
    src.write_bytes(wc.frame(96, 112, 5, 32, "pixel", wc.ref_streams(raster, 32, "pixel"), geo_tags=geo))
    det = ZoneDetector(model, cfg)
    x = det.read(src)
    assert np.array_equal(x.cpu().numpy(), raster)
    want = det.run_to_file(x, tmp_path / "want.tif", source=src)
    out = det.run_files(src, dst)
    assert torch.equal(out, want) and out.shape == (2, 96, 112)
    assert dst.read_bytes() == (tmp_path / "want.tif").read_bytes()
    t = wc.parse_ifd(dst.read_bytes())
    for tag, (typ, cnt, raw) in geo.items():
        assert t[tag][:3] == (typ, cnt, raw), tag
    # a truth file: its first band scores the run as the tensor does
    truth = (wc.labels(1, 96, 112, seed=3, k=C) % C + 1).astype(np.uint8)
    (tmp_path / "truth.tif").write_bytes(rc.build_tiff(truth, rows_per_strip=8, predictor=2))
    det.run_files(src, tmp_path / "scored.tif", truth=tmp_path / "truth.tif", interleave="pixel")
    got = det.window_confmats.clone()
    det.run(x, torch.from_numpy(truth[0]).to(dev))
    assert torch.equal(got, det.window_confmats) and int(got.sum()) > 0
    assert wc.parse_ifd((tmp_path / "scored.tif").read_bytes())[284][3] == (1,)
    # fewer bands than the config's channels ask for
    (tmp_path / "rgb.tif").write_bytes(rc.build_tiff(raster[:3], tile=(32, 32)))
    with pytest.raises(ValueError, match="3 bands"):
        det.read(tmp_path / "rgb.tif")
