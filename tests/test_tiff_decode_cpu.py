"""CPU side of the device TIFF read path (no device needed): the reference decoder of tiff_lzw_decode_cases against PIL / libtiff and
as the inverse of the reference encoder, ``tiff.tiff_strip_layout`` on the files it must accept and the files it must leave to PIL,
the ``decode`` argument of ``metrics`` and the refusals of ``ops.tiff_lzw_decode``."""
import io
import struct

import numpy as np
import pytest
from PIL import Image

import tiff_lzw_cases as tc
import tiff_lzw_decode_cases as dc


def _pil_images():
    rng = np.random.default_rng(0)
    return {"smooth": tc.smooth_mask(), "noise19": tc.noise_mask(), "noise256": rng.integers(0, 256, (512, 512)).astype(np.uint8),
            "constant_64": np.full((64, 64), 7, np.uint8), "40x37": rng.integers(0, 19, (40, 37)).astype(np.uint8),
            "70x700": dc.small_image(70, 700)}


PIL_IMAGES = _pil_images()


def _decode_file(data, decoder=dc.lzw_decode_strip):
    """(pixels, statuses) of a file through tiff_strip_layout and the reference decoder"""
    from flair_amd.tiff import tiff_strip_layout
    lay = tiff_strip_layout(data)
    assert lay is not None
    out, statuses = bytearray(), []
    for k, (off, cnt) in enumerate(zip(lay.offsets, lay.counts)):
        want = min(lay.rows_per_strip, lay.H - k * lay.rows_per_strip) * lay.W
        if lay.compression == 1:
            got, st = data[off:off + want], 0 if cnt >= want else 1
        else:
            got, st = decoder(data[off:off + cnt], want)
        out += got
        statuses.append(st)
    return np.frombuffer(bytes(out), np.uint8).reshape(lay.H, lay.W), statuses, lay


@pytest.mark.parametrize("name", list(PIL_IMAGES))
def test_reference_decoder_reads_pil_files(name):
    img = PIL_IMAGES[name]
    data = dc.pil_file(img, compression="tiff_lzw")
    got, statuses, lay = _decode_file(data)
    assert set(statuses) == {0} and np.array_equal(got, img)
    assert np.array_equal(got, np.asarray(Image.open(io.BytesIO(data))))
    assert lay.rows_per_strip * lay.W <= dc.MAX_STRIP   # PIL's strips are the large class, never more


def test_pil_strips_are_64_kb():
    lay = _decode_file(dc.pil_file(PIL_IMAGES["smooth"], compression="tiff_lzw"))[2]
    assert (lay.rows_per_strip, len(lay.offsets), lay.compression) == (128, 4, 5)


@pytest.mark.parametrize("kind", ["constant", "values19", "values256"])
def test_reference_decoder_inverts_the_reference_encoder(kind):
    """every length at which the encoder switches its width or resets its table, and whole 16 KB strips"""
    row = tc.boundary_row()
    _, lengths = tc.boundary_lengths(row)
    strips = [row[:L].tobytes() for L in lengths + [1, 2, 3]] if kind == "values256" else []
    strips.append({"constant": dc.constant_strip(16384), "values19": dc.values_strip(16384, 19),
                   "values256": dc.values_strip(16384, 256)}[kind])
    for s in strips:
        assert dc.lzw_decode_strip(tc.lzw_strip(s), len(s)) == (s, 0)
        assert dc.lzw_decode_strip(dc.lzw_strip_with_clears(s, 100), len(s)) == (s, 0)
        if len(s) > 8:   # a clipped last string, and the bytes behind the end ignored
            assert dc.lzw_decode_strip(tc.lzw_strip(s) + b"\xff" * 16, len(s) - 5) == (s[:-5], 0)


def test_reference_decoder_statuses():
    C, E = (256, 9), (257, 9)
    s = dc.values_strip(4000, 19)
    enc = tc.lzw_strip(s)
    assert dc.lzw_decode_strip(enc[:len(enc) // 2], len(s))[1] == 1
    assert dc.lzw_decode_strip(b"", 4) == (b"", 1)
    assert dc.lzw_decode_strip(dc.pack_codes([C, E]), 4) == (b"", 2)
    assert dc.lzw_decode_strip(dc.pack_codes([C, (300, 9)]), 4) == (b"", 3)
    assert dc.lzw_decode_strip(dc.pack_codes([C, (65, 9), (400, 9)]), 4) == (b"A", 4)
    assert dc.lzw_decode_strip(dc.pack_codes([C, (65, 9), (258, 9), (259, 9), E]), 6) == (b"AAAAAA", 0)   # code == nxt twice
    assert dc.lzw_decode_strip(dc.pack_codes([C, (65, 9), (258, 9), (259, 9), E]), 7) == (b"AAAAAA", 2)


def _swap_to_mm(data: bytes) -> bytes:
    """a little-endian classic TIFF of SHORT / LONG entries rewritten big-endian by hand (the strips stay where they are)"""
    assert data[:4] == b"II*\0"
    (ifd,) = struct.unpack_from("<I", data, 4)
    out = bytearray(data)
    out[:8] = b"MM\0*" + struct.pack(">I", ifd)
    (n,) = struct.unpack_from("<H", data, ifd)
    struct.pack_into(">H", out, ifd, n)
    for i in range(n):
        at = ifd + 2 + 12 * i
        tag, typ, cnt = struct.unpack_from("<HHI", data, at)
        assert typ in (3, 4)
        struct.pack_into(">HHI", out, at, tag, typ, cnt)
        fmt, size = ("H", 2) if typ == 3 else ("I", 4)
        if size * cnt <= 4:
            vals = struct.unpack_from(f"<{cnt}{fmt}", data, at + 8)
            out[at + 8:at + 12] = struct.pack(f">{cnt}{fmt}", *vals).ljust(4, b"\0")
        else:
            (where,) = struct.unpack_from("<I", data, at + 8)
            struct.pack_into(">I", out, at + 8, where)
            struct.pack_into(f">{cnt}{fmt}", out, where, *struct.unpack_from(f"<{cnt}{fmt}", data, where))
    struct.pack_into(">I", out, ifd + 2 + 12 * n, 0)
    return bytes(out)


def test_layout_accepts():
    from flair_amd.tiff import tiff_strip_layout
    from flair_amd.writer import tiff_lzw_file
    img = PIL_IMAGES["40x37"]
    for R in (40, 8):   # one strip (offset and count inside the entries) and five
        data = tiff_lzw_file(40, 37, R, tc.ref_strips(img, R))
        lay = tiff_strip_layout(data)
        assert (lay.H, lay.W, lay.rows_per_strip, lay.compression, len(lay.offsets)) == (40, 37, R, 5, -(-40 // R))
        assert [data[o:o + c] for o, c in zip(lay.offsets, lay.counts)] == tc.ref_strips(img, R)
        assert np.array_equal(_decode_file(data)[0], img)
        mm = _swap_to_mm(data)
        assert mm[:2] == b"MM" and np.array_equal(np.asarray(Image.open(io.BytesIO(mm))), img)   # libtiff agrees it is a TIFF
        assert tiff_strip_layout(mm) == lay and np.array_equal(_decode_file(mm)[0], img)
    stored = dc.pil_file(img)
    lay = tiff_strip_layout(stored)
    assert lay.compression == 1 and np.array_equal(_decode_file(stored)[0], img)
    assert tiff_strip_layout(memoryview(stored)) == lay and tiff_strip_layout(np.frombuffer(stored, np.uint8)) == lay
    # 128 x 512 is exactly the cap
    assert tiff_strip_layout(dc.pil_file(np.zeros((128, 512), np.uint8), compression="tiff_lzw")) is not None


def test_layout_leaves_to_pil():
    from flair_amd.tiff import MAX_LZW_STRIP, tiff_strip_layout
    from flair_amd.writer import tiff_lzw_file
    assert MAX_LZW_STRIP == dc.MAX_STRIP
    img = PIL_IMAGES["40x37"]
    good = dc.pil_file(img, compression="tiff_lzw")
    assert tiff_strip_layout(good) is not None
    assert tiff_strip_layout(dc.pil_file(img, compression="tiff_adobe_deflate")) is None
    assert tiff_strip_layout(dc.pil_file(np.stack([img, img], axis=-1).astype(np.uint8))) is None           # 2 bands ("LA")
    assert tiff_strip_layout(dc.pil_file(img.astype(np.uint16))) is None
    for cut in (0, 1, 3, 7, 9, 20):
        assert tiff_strip_layout(good[:cut]) is None
    ours = tiff_lzw_file(40, 37, 8, tc.ref_strips(img, 8))
    assert tiff_strip_layout(ours) is not None and tiff_strip_layout(ours[:-1]) is None   # the last strip ends past the end of the file
    assert tiff_strip_layout(ours[:140]) is None                      # the arrays of offsets and counts do
    assert tiff_strip_layout(b"II*\0" + b"\xff" * 64) is None and tiff_strip_layout(b"not a tiff at all") is None
    assert tiff_strip_layout(b"II+\0" + good[4:]) is None             # BigTIFF's magic
    past = bytearray(tiff_lzw_file(40, 37, 40, tc.ref_strips(img, 40)))
    at = 8 + 2 + 12 * 5 + 8                                            # the value of entry 273 of writer.tiff_lzw_file's IFD
    assert struct.unpack_from("<H", past, at - 8)[0] == 273
    struct.pack_into("<I", past, at, len(past))
    assert tiff_strip_layout(bytes(past)) is None
    big = np.zeros((130, 512), np.uint8)                               # one LZW strip of 66 560 decoded bytes: over the cap
    assert tiff_strip_layout(tiff_lzw_file(130, 512, 130, tc.ref_strips(big, 130))) is None
    assert tiff_strip_layout(tiff_lzw_file(130, 512, 128, tc.ref_strips(big, 128))) is not None
    pred2 = dc.pil_file(img, compression="tiff_lzw", tiffinfo={317: 2})
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(pred2))), img) and tiff_strip_layout(pred2) is None   # predictor 2


def test_cap_agrees_between_python_and_c():
    from flair_amd import ops
    assert ops.tiff_lzw_decode_max_strip() == dc.MAX_STRIP


def test_decode_argument(tmp_path, monkeypatch):
    from flair_amd import metrics as M
    monkeypatch.delenv("FLAIR_METRICS_DECODE", raising=False)
    assert M.DECODE_MODES == ("host", "device") and M.DECODE_DEFAULT == "host"
    assert M.resolve_decode(None) == "host" and M.resolve_decode("device") == "device" and M.resolve_decode("host") == "host"
    with pytest.raises(ValueError):
        M.resolve_decode("bogus")
    monkeypatch.setenv("FLAIR_METRICS_DECODE", "device")
    assert M.resolve_decode(None) == "device" and M.resolve_decode("host") == "host"
    monkeypatch.setenv("FLAIR_METRICS_DECODE", "gpu")
    with pytest.raises(ValueError):
        M.resolve_decode(None)
    # metrics() itself resolves the mode before it reads anything: the CSV of this config does not exist
    cfg = {"paths": {"test_csv": str(tmp_path / "absent.csv")}, "classes": {1: [1, "a"], 2: [1, "b"]}}
    with pytest.raises(ValueError, match="decode"):
        M.metrics(cfg, tmp_path / "preds")
    with pytest.raises(ValueError, match="decode"):
        M.metrics(cfg, tmp_path / "preds", decode="pil")
    monkeypatch.delenv("FLAIR_METRICS_DECODE")
    monkeypatch.setattr(M, "DECODE_DEFAULT", "device")
    assert M.resolve_decode(None) == "device"


def test_host_tensors_are_refused():
    import torch
    from flair_amd import ops
    from flair_amd._lib import FlairHipError
    src = torch.zeros(16, dtype=torch.uint8)
    i64, i32 = torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(FlairHipError):
        ops.tiff_lzw_decode(src, i64, i32, i64, i32, i32, 16)
    with pytest.raises(FlairHipError):
        ops.tiff_lzw_decode(src.to(torch.int32), i64, i32, i64, i32, i32, 16)
    with pytest.raises(FlairHipError):
        ops.tiff_lzw_decode(src, i32, i32, i64, i32, i32, 16)   # a table of the wrong type
