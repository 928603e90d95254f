"""Shared cases of the raster writer tests (flair_amd/raster_writer.py, tiff_lzw_encode_tiles_kernel in csrc/tiff_lzw.hip): a numpy
restatement of the byte stream of every TIFF tile (padding, interleave, the fp32 conversion), a small IFD parser that reads tiled
8-bit files of any number of bands back with the reference LZW decoder, the rasters, and helpers that frame a file on the host."""
import struct

import numpy as np

import tiff_lzw_cases as tc
import tiff_lzw_decode_cases as dc
from flair_amd.raster_writer import tiled_tiff_header, tiled_tiff_ifd

FILL = 0xA5
TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 1, 8: 2, 9: 4, 10: 8, 11: 4, 12: 8, 13: 4, 16: 8, 17: 8, 18: 8}
TYPE_FMT = {1: "B", 3: "H", 4: "I", 16: "Q"}


def to_bytes(raster, scale=None):
    """(bands, H, W) uint8 as it is; fp32: uint8(trunc(min(max(v * scale_b, 0), 255))), NaN -> 0, the product in fp32"""
    raster = np.asarray(raster)
    if raster.dtype == np.uint8:
        assert scale is None
        return raster
    assert raster.dtype == np.float32 and len(scale) == raster.shape[0]
    with np.errstate(invalid="ignore"):
        p = raster * np.asarray(scale, dtype=np.float32)[:, None, None]
        assert p.dtype == np.float32
        p = np.where(p > 0, p, np.float32(0))        # NaN compares false
        p = np.where(p < 255, p, np.float32(255))
    return np.trunc(p).astype(np.uint8)


def tile_streams(raster, tile, interleave, scale=None):
    """the byte stream of every TIFF tile, in the order of flair_tiff_lzw_encode_tiles: band: (b * ty + y) * tx + x, T * T bytes of
    band b; pixel: y * tx + x, T * T * bands bytes, the bands of a pixel next to each other.  Pixels outside the raster are 0."""
    u8 = to_bytes(raster, scale)
    bands, H, W = u8.shape
    ty, tx = -(-H // tile), -(-W // tile)
    padded = np.zeros((bands, ty * tile, tx * tile), np.uint8)
    padded[:, :H, :W] = u8
    tiles = padded.reshape(bands, ty, tile, tx, tile)
    if interleave == "band":
        t = tiles.transpose(0, 1, 3, 2, 4).reshape(bands * ty * tx, tile * tile)
    else:
        assert interleave == "pixel"
        t = tiles.transpose(1, 3, 2, 4, 0).reshape(ty * tx, tile * tile * bands)
    return [row.tobytes() for row in t]


def tile_streams_slow(raster, tile, scale=None):
    """pixel interleave, byte by byte from the issue's sentence: byte k of stream (y, x) is row k / (T * bands), column
    (k / bands) % T, band k % bands of the tile"""
    u8 = to_bytes(raster, scale)
    bands, H, W = u8.shape
    ty, tx = -(-H // tile), -(-W // tile)
    out = []
    for y in range(ty):
        for x in range(tx):
            s = bytearray(tile * tile * bands)
            for k in range(len(s)):
                r, c, b = k // (tile * bands), (k // bands) % tile, k % bands
                yy, xx = y * tile + r, x * tile + c
                s[k] = int(u8[b, yy, xx]) if yy < H and xx < W else 0
            out.append(bytes(s))
    return out


def ref_streams(raster, tile, interleave, scale=None):
    return [tc.lzw_strip(s) for s in tile_streams(raster, tile, interleave, scale)]


def frame(H, W, bands, tile, interleave, streams, bigtiff=True, geo_tags=None):
    """a whole file from finished streams with the library's framing, laid out as write_raster lays it out"""
    offsets, parts, at = [], [], 16
    for s in streams:
        offsets.append(at)
        parts.append(s + b"\0" * (-len(s) % 16))
        at += len(parts[-1])
    ifd = tiled_tiff_ifd(H, W, bands, tile, interleave, offsets, [len(s) for s in streams], at, bigtiff=bigtiff, geo_tags=geo_tags)
    return tiled_tiff_header(at, bigtiff).ljust(16, b"\0") + b"".join(parts) + ifd


def parse_ifd(data):
    """{tag: (type, count, raw bytes, values or None)} of the first IFD of a little-endian classic or BigTIFF file, the tags in file
    order under the key "order", and whether the file is a BigTIFF under "bigtiff" """
    assert data[:2] == b"II"
    (magic,) = struct.unpack_from("<H", data, 2)
    if magic == 43:
        assert struct.unpack_from("<HH", data, 4) == (8, 0)
        (ifd,) = struct.unpack_from("<Q", data, 8)
        (n,) = struct.unpack_from("<Q", data, ifd)
        first, fmt, size, inline = ifd + 8, "<HHQ8s", 20, 8
    else:
        assert magic == 42
        (ifd,) = struct.unpack_from("<I", data, 4)
        (n,) = struct.unpack_from("<H", data, ifd)
        first, fmt, size, inline = ifd + 2, "<HHI4s", 12, 4
    tags = {"order": [], "bigtiff": magic == 43}
    for i in range(n):
        tag, typ, cnt, value = struct.unpack_from(fmt, data, first + size * i)
        nbytes = TYPE_SIZE[typ] * cnt
        if nbytes <= inline:
            raw = value[:nbytes]
        else:
            (at,) = struct.unpack("<Q" if magic == 43 else "<I", value)
            assert at + nbytes <= len(data), tag
            raw = bytes(data[at:at + nbytes])
        vals = struct.unpack(f"<{cnt}{TYPE_FMT[typ]}", raw) if typ in TYPE_FMT else None
        tags[tag] = (typ, cnt, raw, vals)
        tags["order"].append(tag)
    nxt = struct.unpack_from("<Q" if magic == 43 else "<I", data, first + size * n)[0]
    assert nxt == 0
    return tags


def read_file(data):
    """(bands, H, W) uint8 of a tiled 8-bit LZW file as raster_writer frames it, every tile through the reference decoder; checks
    the tags a reader depends on along the way"""
    t = parse_ifd(data)
    one = lambda tag: t[tag][3][0]   # noqa: E731
    W, H, bands, T = one(256), one(257), one(277), one(322)
    assert one(323) == T and T % 16 == 0 and one(259) == 5
    assert t[258][3] == (8,) * bands and t[339][3] == (1,) * bands
    # three bands are RGB (GDAL's own choice for three 8-bit bands, and the one layout of several bands PIL reads whole); of any
    # other number the first is grey and the rest are extra samples of unspecified meaning
    if bands == 3:
        assert one(262) == 2 and 338 not in t
    else:
        assert one(262) == 1 and (338 in t) == (bands > 1) and (bands == 1 or t[338][3] == (0,) * (bands - 1))
    planar = one(284)
    ty, tx = -(-H // T), -(-W // T)
    offsets, counts = t[324][3], t[325][3]
    want_type = 16 if t["bigtiff"] else 4
    assert t[324][0] == want_type and t[325][0] == want_type
    n = (bands if planar == 2 else 1) * ty * tx
    assert len(offsets) == len(counts) == n
    samples = 1 if planar == 2 else bands
    tiles = []
    for off, cnt in zip(offsets, counts):
        assert off % 16 == 0 and 16 <= off and off + cnt <= len(data)
        px, status = dc.lzw_decode_strip(bytes(data[off:off + cnt]), T * T * samples)
        assert status == 0
        tiles.append(np.frombuffer(px, np.uint8))
    a = np.stack(tiles)
    if planar == 2:
        full = a.reshape(bands, ty, tx, T, T).transpose(0, 1, 3, 2, 4).reshape(bands, ty * T, tx * T)
    else:
        full = a.reshape(ty, tx, T, T, bands).transpose(4, 0, 2, 1, 3).reshape(bands, ty * T, tx * T)
    assert not full[:, H:, :].any() and not full[:, :, W:].any()   # the padding of the edge tiles
    return full[:, :H, :W]


def patch_extra_samples(data, value=2):
    """a copy of a 2-band file whose one ExtraSamples SHORT reads ``value`` (2: unassociated alpha, which PIL opens as LA)"""
    t = parse_ifd(data)
    assert t[338][1] == 1 and t[338][3] == (0,)
    data = bytearray(data)
    if t["bigtiff"]:
        (ifd,) = struct.unpack_from("<Q", data, 8)
        at = ifd + 8 + 20 * t["order"].index(338) + 12
    else:
        (ifd,) = struct.unpack_from("<I", data, 4)
        at = ifd + 2 + 12 * t["order"].index(338) + 8
    struct.pack_into("<H", data, at, value)
    return bytes(data)


def pil_read(data):
    """(bands, H, W) as PIL / libtiff read the file: 1 band (L), 3 bands (RGB), 2 chunky bands with ExtraSamples patched (LA)"""
    import io
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    a = np.asarray(im)
    return im.mode, (a[None] if a.ndim == 2 else a.transpose(2, 0, 1))


def labels(bands, H, W, seed=3, k=19):
    """label-like bytes: runs of equal values with 10 % of the pixels redrawn, another seed per band"""
    rng = np.random.default_rng(seed)
    m = np.kron(rng.integers(0, k, (bands, -(-H // 8), -(-W // 8))), np.ones((1, 8, 8), np.int64))[:, :H, :W]
    salt = rng.random(m.shape) < 0.1
    m[salt] = rng.integers(0, 256, int(salt.sum()))
    return np.ascontiguousarray(m.astype(np.uint8))


def noise(bands, H, W, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (bands, H, W)).astype(np.uint8)


def argmax_raster(H=40, W=56, seed=8):
    """fp32 (2, H, W) as ZoneDetector.run returns for 'argmax': classes 0 .. 18, confidences with every value the conversion to a
    byte can trip over: 0, 1, 0.5, the fp32 neighbours of 1 and of k / 255, values outside [0, 1] and NaN"""
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, 19, (H, W)).astype(np.float32)
    conf = rng.random((H, W)).astype(np.float32)
    special = [0.0, 1.0, 0.5, np.nextafter(np.float32(1), np.float32(0)), -0.1, 1.5, np.nan, -0.0, np.inf, -np.inf, 1e-30, 255.0, 256.0]
    for k in (1, 2, 3, 51, 85, 127, 128, 170, 200, 254, 255):
        v = np.float32(k) / np.float32(255)
        special += [v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(2))]
    conf.reshape(-1)[:len(special)] = np.array(special, dtype=np.float32)
    conf.reshape(-1)[-len(special):] = np.array(special, dtype=np.float32)[::-1]   # and in a padded edge tile's row
    return np.stack([cls, conf])


ARGMAX_SCALE = (1.0, 255.0)


def smooth_blobs(H=520, W=530):
    """one band of tc.smooth_mask's blobs, tiled out to (H, W)"""
    m = tc.smooth_mask()
    return np.ascontiguousarray(np.tile(m, (-(-H // 512), -(-W // 512)))[None, :H, :W])


# name -> (raster, tile, interleave, scale): what the kernel's streams are compared on, stream for stream
def kernel_cases():
    cases = {}
    for H, W in ((40, 56), (37, 53)):
        for bands in (1, 3, 13):
            for il in ("band", "pixel"):
                cases[f"labels_{H}x{W}_b{bands}_{il}"] = (labels(bands, H, W, seed=H + bands), 16, il, None)
    cases["noise_64_T64"] = (noise(1, 64, 64), 64, "band", None)
    cases["noise_128_T128"] = (noise(1, 128, 128, seed=6), 128, "band", None)
    cases["b19_48_pixel"] = (labels(19, 48, 48, seed=19), 16, "pixel", None)
    cases["constant"] = (np.full((2, 40, 56), 7, np.uint8), 16, "band", None)
    cases["constant_pixel"] = (np.full((2, 40, 56), 7, np.uint8), 16, "pixel", None)
    cases["argmax_f32_band"] = (argmax_raster(), 16, "band", ARGMAX_SCALE)
    cases["argmax_f32_pixel"] = (argmax_raster(), 16, "pixel", ARGMAX_SCALE)
    return cases


def geo_source(bigtiff=False, order="<"):
    """a tiny stored TIFF with GeoTIFF tags 33550 / 33922 / 34735 / 34737 (and one tag that is none), framed by hand; returns
    (file bytes, {tag: (type, count, little-endian raw bytes)})"""
    e = order
    scale = (0.2, 0.2, 0.0)
    tie = (0.0, 0.0, 0.0, 880000.0, 6520000.0, 0.0)
    keys = (1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, 2154)
    ascii_ = b"RGF93 / Lambert-93|\0"
    geo = [(33550, 12, 3, "d", scale), (33922, 12, 6, "d", tie), (34735, 3, 16, "H", keys), (34737, 2, len(ascii_), None, ascii_)]
    want = {tag: (typ, cnt, struct.pack(f"<{cnt}{f}", *v) if f else v) for tag, typ, cnt, f, v in geo}
    base = [(256, 3, 1, "H", (2,)), (257, 3, 1, "H", (2,)), (258, 3, 1, "H", (8,)), (259, 3, 1, "H", (1,)), (262, 3, 1, "H", (1,)),
            (273, 4, 1, "I", (None,)), (277, 3, 1, "H", (1,)), (278, 3, 1, "H", (2,)), (279, 4, 1, "I", (4,)),
            (305, 2, 5, None, b"test\0")]
    entries = sorted(base + geo)
    inline, esize, cfmt, ofmt = (8, 20, "Q", "Q") if bigtiff else (4, 12, "H", "I")
    hdr = 16 if bigtiff else 8
    pixels_at = hdr
    ifd = pixels_at + 4
    tail_at = ifd + struct.calcsize(cfmt) + esize * len(entries) + inline
    head, tail = [struct.pack(e + cfmt, len(entries))], []
    for tag, typ, cnt, f, v in entries:
        if tag == 273:
            v = (pixels_at,)
        raw = struct.pack(f"{e}{cnt}{f}", *v) if f else v
        if len(raw) <= inline:
            value = raw.ljust(inline, b"\0")
        else:
            value = struct.pack(e + ofmt, tail_at)
            tail.append(raw + b"\0" * (len(raw) % 2))
            tail_at += len(tail[-1])
        head.append(struct.pack(f"{e}HH{ofmt}", tag, typ, cnt) + value)
    head.append(b"\0" * inline)
    order_mark = b"II" if e == "<" else b"MM"
    header = (struct.pack(e + "2sHHHQ", order_mark, 43, 8, 0, ifd) if bigtiff else struct.pack(e + "2sHI", order_mark, 42, ifd))
    return header + bytes([1, 2, 3, 4]) + b"".join(head + tail), want
