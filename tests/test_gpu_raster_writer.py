"""tiff_lzw_encode_tiles_kernel and tiff_pack_streams_kernel (csrc/tiff_lzw.hip) through the C ABI and flair_amd.ops, and
raster_writer.write_raster / ZoneDetector.write on top of them: every tile's stream equals the reference encoder's of the restated
tile bytes, nothing is written outside a slot or a packed stream, and the files read back, with PIL / libtiff where they can read the
layout and with the reference decoder otherwise, to the raster."""
import threading

import numpy as np
import pytest
import torch

import raster_writer_cases as rc
import tiff_lzw_cases as tc

pytestmark = pytest.mark.gpu

CASES = rc.kernel_cases()


def _encode(dev, raster, tile, interleave, scale=None, first=0, n=None, extra_slots=1):
    """the C ABI on a 0xA5-filled buffer of n + extra_slots slots: (streams, counts, the whole buffer, slot_bytes)"""
    from flair_amd import _lib as L
    from flair_amd import ops
    lib = L.lib()
    bands, H, W = raster.shape
    total = ops.tiff_tile_streams(bands, H, W, tile, interleave)
    n = total - first if n is None else n
    samples = bands if interleave == "pixel" else 1
    slot = lib.flair_tiff_lzw_tile_slot_bytes(tile, samples)
    assert slot == tc.slot_bytes(1, tile * tile * samples)
    x = torch.from_numpy(np.ascontiguousarray(raster)).to(dev)
    sc = None if scale is None else torch.tensor(scale, dtype=torch.float32).to(dev)
    out = torch.full(((n + extra_slots) * slot,), rc.FILL, dtype=torch.uint8, device=dev)
    counts = torch.full((n + extra_slots,), -1, dtype=torch.int32, device=dev)
    L.check(lib.flair_tiff_lzw_encode_tiles(L.ptr(x), int(raster.dtype == np.float32), L.ptr(sc), bands, H, W, tile,
                                            ops.TIFF_INTERLEAVE[interleave], first, n, L.ptr(out), slot, L.ptr(counts), L.stream()),
            "flair_tiff_lzw_encode_tiles")
    out_h, counts_h = out.cpu().numpy(), counts.cpu().numpy()
    assert (counts_h[n:] == -1).all() and (counts_h[:n] > 0).all() and (counts_h[:n] <= slot).all()
    streams = [out_h[i * slot:][:counts_h[i]].tobytes() for i in range(n)]
    return streams, counts_h[:n], out_h, slot


def _assert_streams(got, want, what=""):
    assert [len(g) for g in got] == [len(w) for w in want], what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{what} stream {i}: first difference at byte {next(k for k, (p, q) in enumerate(zip(g, w)) if p != q)} of {len(w)}"


def _assert_guards(out, counts, slot):
    """slots past the last stream keep their fill, and so do the bytes of a slot past its stream (rounded up to a 32-bit word)"""
    n = len(counts)
    assert (out[n * slot:] == rc.FILL).all()
    for i, c in enumerate(counts):
        assert (out[i * slot + (c + 3) // 4 * 4:(i + 1) * slot] == rc.FILL).all(), i


@pytest.mark.parametrize("name", sorted(CASES))
def test_streams_equal_the_reference_encoder(dev, name):
    raster, tile, interleave, scale = CASES[name]
    streams, counts, out, slot = _encode(dev, raster, tile, interleave, scale)
    _assert_streams(streams, rc.ref_streams(raster, tile, interleave, scale), name)
    _assert_guards(out, counts, slot)


def test_a_window_of_streams(dev):
    """first_stream / n_streams: the same bytes as those streams of a full call, in slots counted from the window's start"""
    for name, first, n in (("labels_37x53_b13_band", 17, 40), ("labels_37x53_b13_band", 155, 1), ("labels_40x56_b3_pixel", 5, 6),
                           ("argmax_f32_band", 11, 9)):
        raster, tile, interleave, scale = CASES[name]
        want = rc.ref_streams(raster, tile, interleave, scale)
        streams, counts, out, slot = _encode(dev, raster, tile, interleave, scale, first=first, n=n, extra_slots=2)
        _assert_streams(streams, want[first:first + n], name)
        _assert_guards(out, counts, slot)


@pytest.mark.parametrize("interleave", ["band", "pixel"])
def test_samples_past_2_31(dev, interleave):
    """a raster of more than 2^31 bytes: the last two streams, whose samples lie past that index, padded at both edges"""
    from flair_amd import ops
    H, W, T = 16395, 65549, 16
    assert (H + 16384) * W > 2 ** 31                      # band 1 of the last tile row lies past 2^31
    corner = rc.noise(2, H - 16384, W - 65520, seed=31)     # rows 16384 .., columns 65520 ..: the last tile row's last two tiles
    x = torch.zeros(2, H, W, dtype=torch.uint8, device=dev)
    x[:, 16384:, 65520:] = torch.from_numpy(corner).to(dev)
    total = ops.tiff_tile_streams(2, H, W, T, interleave)
    slots, counts = ops.tiff_lzw_encode_tiles(x, T, interleave, first_stream=total - 2, n_streams=2)
    s, c = slots.cpu().numpy(), counts.cpu().numpy()
    want = rc.ref_streams(corner, T, interleave)[-2:]
    _assert_streams([s[i, :c[i]].tobytes() for i in range(2)], want, interleave)


def test_ops_wrapper(dev):
    from flair_amd import ops
    raster, tile, interleave, scale = CASES["argmax_f32_pixel"]
    slots, counts = ops.tiff_lzw_encode_tiles(torch.from_numpy(raster).to(dev), tile, interleave, scale=scale)
    want = rc.ref_streams(raster, tile, interleave, scale)
    assert slots.shape == (len(want), ops.tiff_lzw_tile_slot_bytes(tile, 2)) and counts.shape == (len(want),)
    s, c = slots.cpu().numpy(), counts.cpu().numpy()
    _assert_streams([s[i, :c[i]].tobytes() for i in range(len(want))], want)
    raster, tile, interleave, _ = CASES["labels_40x56_b3_band"]
    x = torch.from_numpy(raster).to(dev)
    slots, counts = ops.tiff_lzw_encode_tiles(x, tile, first_stream=30, n_streams=4)
    s, c = slots.cpu().numpy(), counts.cpu().numpy()
    _assert_streams([s[i, :c[i]].tobytes() for i in range(4)], rc.ref_streams(raster, tile, "band")[30:34])
    with pytest.raises(ValueError):
        ops.tiff_lzw_encode_tiles(x, tile, first_stream=30, n_streams=7)   # 36 streams
    with pytest.raises(ValueError):
        ops.tiff_lzw_encode_tiles(x, tile, n_streams=0)


def test_encode_argument_errors_launch_nothing(dev):
    from flair_amd import _lib as L
    lib = L.lib()
    bands, H, W, T = 2, 40, 56, 16
    slot = lib.flair_tiff_lzw_tile_slot_bytes(T, 1)
    n = bands * 3 * 4
    x = torch.zeros(bands, H, W, dtype=torch.uint8, device=dev)
    xf = torch.zeros(bands, H, W, dtype=torch.float32, device=dev)
    sc = torch.ones(bands, dtype=torch.float32, device=dev)
    out = torch.full((n * slot,), rc.FILL, dtype=torch.uint8, device=dev)
    counts = torch.full((n,), -1, dtype=torch.int32, device=dev)
    px, pf, ps, po, pc, st = L.ptr(x), L.ptr(xf), L.ptr(sc), L.ptr(out), L.ptr(counts), L.stream()
    f = lib.flair_tiff_lzw_encode_tiles
    assert f(None, 0, None, bands, H, W, T, 0, 0, n, po, slot, pc, st) == -1
    assert f(px, 0, None, bands, H, W, T, 0, 0, n, None, slot, pc, st) == -1
    assert f(px, 0, None, bands, H, W, T, 0, 0, n, po, slot, None, st) == -1
    assert f(pf, 1, None, bands, H, W, T, 0, 0, n, po, slot, pc, st) == -1        # fp32 without a scale
    assert f(px, 0, None, 0, H, W, T, 0, 0, n, po, slot, pc, st) == -1
    assert f(px, 0, None, bands, 0, W, T, 0, 0, n, po, slot, pc, st) == -1
    assert f(px, 0, None, bands, H, W, 24, 0, 0, n, po, slot, pc, st) == -1       # tile no multiple of 16
    assert f(px, 0, None, bands, H, W, 0, 0, 0, n, po, slot, pc, st) == -1
    assert f(px, 0, None, bands, H, W, T, 2, 0, n, po, slot, pc, st) == -1
    assert f(px, 2, None, bands, H, W, T, 0, 0, n, po, slot, pc, st) == -1
    assert f(px, 0, None, bands, H, W, T, 0, 0, 0, po, slot, pc, st) == -1        # an empty window
    assert f(px, 0, None, bands, H, W, T, 0, -1, 2, po, slot, pc, st) == -1
    assert f(px, 0, None, bands, H, W, T, 0, n - 1, 2, po, slot, pc, st) == -1    # a window past the last stream
    assert f(px, 0, None, bands, H, W, T, 1, 0, n, po, slot, pc, st) == -1        # pixel interleave has 12 streams
    assert f(px, 0, None, bands, H, W, T, 0, 0, n, po, slot - 16, pc, st) == -100
    assert f(px, 0, None, bands, H, W, T, 1, 0, 12, po, slot, pc, st) == -100     # a pixel-interleaved slot holds two bands
    assert f(px, 0, None, bands, H, W, T, 0, 0, n, po + 4, slot, pc, st) == -2
    assert f(px, 0, None, bands, H, W, T, 0, 0, n, po, slot + 8, pc, st) == -2
    assert lib.flair_tiff_lzw_tile_slot_bytes(T, 0) == -1 and lib.flair_tiff_lzw_tile_slot_bytes(0, 1) == -1
    assert lib.flair_tiff_lzw_tile_slot_bytes(32768, 2) == -1                      # more than 2^30 bytes in a stream
    torch.cuda.synchronize()
    assert (out.cpu() == rc.FILL).all() and (counts.cpu() == -1).all()
    assert f(pf, 1, ps, bands, H, W, T, 0, 0, n, po, slot, pc, st) == 0
    assert (counts.cpu() > 0).all()


def _pack_case(dev):
    from flair_amd import ops
    raster, tile, interleave, _ = CASES["labels_37x53_b13_band"]
    want = rc.ref_streams(raster, tile, interleave)
    slots, counts = ops.tiff_lzw_encode_tiles(torch.from_numpy(raster).to(dev), tile, interleave)
    return want, slots, counts, ops.tiff_lzw_tile_slot_bytes(tile, 1)


def test_pack_streams(dev):
    from flair_amd import ops
    want, slots, counts, slot = _pack_case(dev)
    lens = np.array([len(w) for w in want])
    assert len({int(v) % 16 for v in lens}) > 8          # tails of many lengths, 0 among them or not
    rounded = (lens + 15) & ~15
    offs = np.cumsum(rounded) - rounded
    expect = np.zeros(int(rounded.sum()), np.uint8)
    for o, w in zip(offs, want):
        expect[o:o + len(w)] = np.frombuffer(w, np.uint8)
    payload, offsets = ops.tiff_pack_streams(slots, counts, slot)
    assert offsets.dtype == torch.int64 and offsets.cpu().numpy().tolist() == offs.tolist()
    assert payload.dtype == torch.uint8 and np.array_equal(payload.cpu().numpy(), expect)   # gaps zero
    # into a caller's buffer: the same bytes, and everything behind the last stream keeps its fill
    out = torch.full((len(want) * slot + 256,), rc.FILL, dtype=torch.uint8, device=dev)
    got, offsets2 = ops.tiff_pack_streams(slots, counts, slot, out=out)
    assert got is out and torch.equal(offsets2, offsets)
    h = out.cpu().numpy()
    assert np.array_equal(h[:expect.size], expect) and (h[expect.size:] == rc.FILL).all()
    with pytest.raises(Exception):
        ops.tiff_pack_streams(slots, counts, slot, out=torch.empty(len(want) * slot - 16, dtype=torch.uint8, device=dev))


def test_pack_streams_refusals(dev):
    """a zero-length group and broken arguments launch nothing; a stream whose offset or count breaks the contract is skipped"""
    from flair_amd import _lib as L
    from flair_amd import ops
    lib = L.lib()
    want, slots, counts, slot = _pack_case(dev)
    n = len(want)
    with pytest.raises(ValueError):
        ops.tiff_pack_streams(slots[:0], counts[:0], slot)
    dst = torch.full((n * slot,), rc.FILL, dtype=torch.uint8, device=dev)
    off = torch.arange(n, dtype=torch.int64, device=dev) * slot
    ps, pc, po, pd, st = L.ptr(slots), L.ptr(counts), L.ptr(off), L.ptr(dst), L.stream()
    f = lib.flair_tiff_pack_streams
    assert f(ps, slot, pc, po, 0, pd, dst.numel(), st) == -1
    assert f(ps, slot, pc, po, -3, pd, dst.numel(), st) == -1
    assert f(None, slot, pc, po, n, pd, dst.numel(), st) == -1
    assert f(ps, slot, None, po, n, pd, dst.numel(), st) == -1
    assert f(ps, slot, pc, None, n, pd, dst.numel(), st) == -1
    assert f(ps, slot, pc, po, n, None, dst.numel(), st) == -1
    assert f(ps, 0, pc, po, n, pd, dst.numel(), st) == -1
    assert f(ps, slot, pc, po, n, pd, -1, st) == -1
    assert f(ps + 4, slot, pc, po, n, pd, dst.numel(), st) == -2
    assert f(ps, slot + 8, pc, po, n, pd, dst.numel(), st) == -2
    assert f(ps, slot, pc, po, n, pd + 8, dst.numel(), st) == -2
    torch.cuda.synchronize()
    assert (dst.cpu() == rc.FILL).all()
    # device-side contract: stream 1 at an offset that is no multiple of 16, stream 2 past the end, stream 3 with a count above the
    # slot, stream 4 at a negative offset: none of them is copied, the others are
    bad_off, bad_cnt = off.clone(), counts.clone()
    bad_off[1] += 8
    bad_off[2] = dst.numel() - 16
    bad_cnt[3] = slot + 1
    bad_off[4] = -16
    lens = counts.cpu().numpy()
    assert lens[2] > 16
    assert f(ps, slot, L.ptr(bad_cnt), L.ptr(bad_off), n, pd, dst.numel(), st) == 0
    h = dst.cpu().numpy().reshape(n, slot)
    for i, w in enumerate(want):
        if i in (1, 2, 3, 4):
            assert (h[i] == rc.FILL).all(), i
        else:
            r = -(-len(w) // 16) * 16
            assert h[i, :len(w)].tobytes() == w and not h[i, len(w):r].any() and (h[i, r:] == rc.FILL).all(), i


def _write(tmp_path, dev, name, raster, tile, interleave, **kw):
    from flair_amd.raster_writer import write_raster
    path = tmp_path / name
    info = write_raster(path, torch.from_numpy(raster).to(dev), tile, interleave=interleave, **kw)
    data = path.read_bytes()
    assert info["file_bytes"] == len(data) and info["streams"] == len(rc.tile_streams(raster, tile, interleave, kw.get("scale")))
    assert not [t for t in threading.enumerate() if t.name == "flair-raster-write"]
    return data, info


@pytest.mark.parametrize("bigtiff", [True, False], ids=["bigtiff", "classic"])
def test_written_files_read_back(dev, tmp_path, bigtiff):
    for bands, interleave in ((1, "band"), (3, "band"), (3, "pixel"), (2, "pixel"), (2, "band"), (13, "band"), (13, "pixel")):
        raster = rc.labels(bands, 37, 53, seed=40 + bands)
        data, info = _write(tmp_path, dev, f"b{bands}_{interleave}.tif", raster, 16, interleave, bigtiff=bigtiff)
        # byte for byte the file the host frames from the reference encoder's streams
        assert data == rc.frame(37, 53, bands, 16, interleave, rc.ref_streams(raster, 16, interleave), bigtiff=bigtiff)
        assert info["groups"] == 1
        if bands == 1:
            assert rc.pil_read(data)[0] == "L" and np.array_equal(rc.pil_read(data)[1], raster)
        elif bands == 3:
            mode, px = rc.pil_read(data)
            assert mode == "RGB" and np.array_equal(px, raster)
        elif bands == 2 and interleave == "pixel":
            mode, px = rc.pil_read(rc.patch_extra_samples(data))
            assert mode == "LA" and np.array_equal(px, raster)
        else:
            assert np.array_equal(rc.read_file(data), raster)


def test_file_does_not_depend_on_the_grouping(dev, tmp_path):
    raster = rc.labels(13, 40, 56, seed=77)
    # 156 streams of 256 bytes (band) or 12 of 3 328 (pixel), 4 to a tile row: a third of the streams per group, one tile row per
    # group (5 streams' worth of bytes, cut down to the row), one stream per group
    for interleave, unit, third in (("band", 256, 52), ("pixel", 256 * 13, 4)):
        one, info1 = _write(tmp_path, dev, "one.tif", raster, 16, interleave)
        assert info1["groups"] == 1 and np.array_equal(rc.read_file(one), raster)
        for group_bytes, groups in ((unit * third, 3), (unit * 5, info1["streams"] // 4), (1, info1["streams"])):
            many, info = _write(tmp_path, dev, "many.tif", raster, 16, interleave, group_bytes=group_bytes)
            assert info["groups"] == groups >= 3, (interleave, group_bytes, info)
            assert many == one, (interleave, group_bytes)
    f32 = rc.argmax_raster()
    one, _ = _write(tmp_path, dev, "f32.tif", f32, 16, "band", scale=rc.ARGMAX_SCALE)
    many, info = _write(tmp_path, dev, "f32m.tif", f32, 16, "band", scale=rc.ARGMAX_SCALE, group_bytes=256 * 8)
    assert info["groups"] == 3 and many == one
    assert np.array_equal(rc.read_file(one), rc.to_bytes(f32, rc.ARGMAX_SCALE))


def test_real_size_tiles(dev, tmp_path):
    """520 x 530 at T = 512: four streams of 256 KB, three of them mostly padding, through PIL / libtiff"""
    raster = rc.smooth_blobs()
    assert raster.shape == (1, 520, 530)
    data, info = _write(tmp_path, dev, "real.tif", raster, 512, "band")
    assert info["streams"] == 4
    mode, px = rc.pil_read(data)
    assert mode == "L" and np.array_equal(px, raster)
    t = rc.parse_ifd(data)
    assert t[322][3] == (512,) and all(o % 16 == 0 for o in t[324][3]) and info["payload_bytes"] == sum(t[325][3])


def test_a_worker_error_surfaces_and_no_thread_stays(dev):
    from flair_amd.raster_writer import write_raster
    x = torch.from_numpy(rc.noise(3, 128, 128)).to(dev)
    with pytest.raises(OSError):
        write_raster("/dev/full", x, 16, group_bytes=128 * 128)   # three groups; the device accepts no byte
    assert not [t for t in threading.enumerate() if t.name == "flair-raster-write"]
    with pytest.raises(ValueError):
        write_raster("/dev/null", x, 24)
    with pytest.raises(ValueError):
        write_raster("/dev/null", x.float(), 16)                 # fp32 without a scale
    assert write_raster("/dev/null", x, 16)["streams"] == 3 * 64  # and the writer works after all of that


@pytest.fixture(scope="module")
def zone(dev):
    import flair_amd
    C = 13
    torch.manual_seed(5)
    model = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=C, compute_dtype="f32").to(dev).eval()
    cfg = {"img_pixels_detection": 64, "margin": 8, "output_type": "argmax", "n_classes": C, "batch_size": 4, "channels": [1, 2, 3, 4, 5],
           "norma_task": [{"norm_type": "scaling"}]}
    raster = torch.from_numpy(np.random.default_rng(12).integers(0, 256, size=(5, 96, 96), dtype=np.uint8)).to(dev)
    return model, cfg, raster


def test_zone_detector_run_to_file(dev, tmp_path, zone):
    from flair_amd.zone_detect import ZoneDetector
    model, cfg, raster = zone
    det = ZoneDetector(model, cfg)
    want = det.run(raster)
    src, geo = rc.geo_source()
    (tmp_path / "source.tif").write_bytes(src)
    out = det.run_to_file(raster, tmp_path / "argmax.tif", source=tmp_path / "source.tif")
    assert torch.equal(out, want) and out.shape == (2, 96, 96) and out.dtype == torch.float32
    data = (tmp_path / "argmax.tif").read_bytes()
    t = rc.parse_ifd(data)
    assert t["bigtiff"] and t[322][3] == (64,) and t[277][3] == (2,) and t[284][3] == (2,)
    for tag, (typ, cnt, raw) in geo.items():
        assert t[tag][:3] == (typ, cnt, raw), tag
    got = rc.read_file(data)
    o = out.cpu().numpy()
    assert np.array_equal(got[0], o[0].astype(np.uint8)) and (o[0] == np.trunc(o[0])).all() and o[0].max() < 13
    assert np.array_equal(got, rc.to_bytes(o, (1.0, 255.0)))          # band 1: uint8(p * 255), DESIGN §8 W1
    assert got[1].min() >= 255 // 13                                     # a confidence byte (the largest of 13 probabilities), not 0 / 1
    # write() alone, pixel interleave, no source: no geo tags; the chunky file is one PIL reads once ExtraSamples says alpha
    det.write(out, tmp_path / "chunky.tif", interleave="pixel", bigtiff=False)
    chunky = (tmp_path / "chunky.tif").read_bytes()
    assert not set(rc.parse_ifd(chunky)["order"]) & set(geo)
    mode, px = rc.pil_read(rc.patch_extra_samples(chunky))
    assert mode == "LA" and np.array_equal(px, got)
    with pytest.raises(ValueError):
        det.write(out[:1], tmp_path / "x.tif")
    with pytest.raises(ValueError):
        det.write(out.to(torch.uint8), tmp_path / "x.tif")


def test_zone_detector_class_prob_to_file(dev, tmp_path, zone):
    from flair_amd.zone_detect import ZoneDetector
    model, cfg, raster = zone
    det = ZoneDetector(model, dict(cfg, output_type="class_prob"))
    out = det.run_to_file(raster, tmp_path / "prob.tif")
    assert out.shape == (13, 96, 96) and out.dtype == torch.uint8 and torch.equal(out, det.run(raster))
    data = (tmp_path / "prob.tif").read_bytes()
    assert rc.parse_ifd(data)[277][3] == (13,)
    assert np.array_equal(rc.read_file(data), out.cpu().numpy())
    with pytest.raises(ValueError):
        det.write(out.float(), tmp_path / "x.tif")
