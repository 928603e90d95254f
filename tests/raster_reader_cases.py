"""Shared cases of the raster reader tests (flair_amd/raster_reader.py, csrc/tiff_read.hip): a CPU restatement of the position-based
decode that lists where every table code's string is copied from (and replays the kernel's ring, flush and read-back rules), byte
streams that place those sources on every side of the boundaries the kernel treats specially, a numpy restatement of
flair_tiff_chunks_to_planes, and a host framer of TIFFs of the whole family raster_layout accepts (and of files it must refuse)."""
import functools
import struct

import numpy as np

import raster_writer_cases as wc
import tiff_lzw_cases as tc
import tiff_lzw_decode_cases as dc

FILL = 0xA5
GUARD = 128            # the slot alignment the kernel asks for
BLOCK = 128            # the decoder's flush unit
MAXSTR = 4096          # the ring is window + MAXSTR bytes


def trace_decode(data: bytes, want: int, window=None):
    """(bytes, status, refs) of the position-based decode: the table holds (position, length) into the output and a code is a copy
    from there.  refs lists, per table code, (output position, source position, source length); for code == nxt the source is
    string(old), the last byte being its first byte again.  With ``window`` the copy follows the kernel's rules to the letter: the
    ring of window + MAXSTR bytes, whole blocks flushed to the slot after every code, sources below op - window read back from the
    slot; it asserts that such a source is flushed, and that a ring place still holds the position it is read for."""
    nbits = 8 * len(data)
    word = int.from_bytes(data, "big")
    out, refs = bytearray(), []
    tpos, tlen = {}, {}
    nxt, width, pos, old_pos, old_len = 258, 9, 0, 0, 0
    ring_n = (window or 0) + MAXSTR
    ring, owner, slot, flushed = bytearray(ring_n), [-1] * ring_n, bytearray(), 0

    def put(p, v):
        out.append(v)
        if window:
            ring[p % ring_n], owner[p % ring_n] = v, p

    def get(p, op):
        if not window:
            return out[p]
        if p >= op - window:
            assert owner[p % ring_n] == p, (p, op)
            return ring[p % ring_n]
        assert p < flushed and flushed % BLOCK == 0
        return slot[p]

    def done(status):
        if window:
            assert bytes(slot) == bytes(out[:flushed])
        return bytes(out[:want]), status, refs

    while True:
        op = len(out)
        if op >= want:
            return done(0)
        if pos + width > nbits:
            return done(1)
        code = (word >> (nbits - pos - width)) & ((1 << width) - 1)
        pos += width
        if code == 256:
            nxt, width, old_len = 258, 9, 0
            continue
        if code == 257:
            return done(2)
        if old_len == 0:
            if code >= 256:
                return done(3)
            put(op, code)
            n = 1
        else:
            frm, ln, wrap = 0, 1, None
            if code >= 256:
                if code < nxt:
                    frm, ln = tpos[code], tlen[code]
                elif code == nxt and nxt < 4096:
                    frm, ln, wrap = old_pos, old_len + 1, old_len
                else:
                    return done(4)
            n = min(ln, want - op)
            if code < 256:
                put(op, code)
            else:
                refs.append((op, frm, min(n, ln if wrap is None else wrap)))
                for j in range(n):
                    put(op + j, get(frm + (j if wrap is None or j < wrap else 0), op))
            if nxt < 4096:
                tpos[nxt], tlen[nxt] = old_pos, old_len + 1
                nxt += 1
                if nxt in (511, 1023, 2047):
                    width += 1
        old_pos, old_len = op, n
        if window:
            flushed = (op + n) // BLOCK * BLOCK
            slot += out[len(slot):flushed]


def boundary_counts(refs, window):
    """how many sources lie on each side of the kernel's two boundaries at their code's output position op.  The window, op - window:
    'back' wholly below it (read back from the slot), 'ring' wholly at or above it, 'across' both.  The flush block, op rounded down
    to BLOCK (what is below is in the slot already): 'flushed', 'unflushed', 'half'.  'far': sources more than 65 536 bytes back, the
    strip decoder's whole reach (tiff_lzw_decode_kernel's 16-bit positions); 'longest': the longest source."""
    c = dict(back=0, ring=0, across=0, flushed=0, unflushed=0, half=0, far=0, longest=0)
    for op, frm, n in refs:
        lo, fl = op - window, op // BLOCK * BLOCK
        c["back" if frm + n <= lo else "ring" if frm >= lo else "across"] += 1
        c["flushed" if frm + n <= fl else "unflushed" if frm >= fl else "half"] += 1
        c["far"] += op - frm > 65536
        c["longest"] = max(c["longest"], n)
    return c


def _rand(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def window_streams(window):
    """name -> bytes whose table codes reach back to both sides of ``window`` and across it.  A block of random bytes, a run of n equal
    bytes (which takes about sqrt(2 n) table entries, so the block's pairs stay in the table) and the block again: every pair of the
    second block is copied from exactly n + 300 bytes back."""
    a, b = _rand(300, 21), _rand(300, 22)
    zeros = lambda n: bytes(n)   # noqa: E731
    cases = {
        "far_80000": a + zeros(80000) + a,                                       # > 65 536 back: positions need 32 bits
        "far_repeat": (a + zeros(2 * window)) * 3 + a,                           # a read-back, new output, a read-back: the fence again
        "noise_gap": a + zeros(window // 2) + b + zeros(window) + a + b,         # a noise gap inside the run
        # the first run's longest string (110 bytes, made near its end) is what the second run begins with, window + 50 bytes later:
        # a source across the edge that takes two 64-byte steps (found with the tracer; the CPU test asserts it)
        "long_across": zeros(6000) + a + b"\1" * (window - 300 - 60) + zeros(6000),
    }
    for d in (-1, 0, 1, 2, 3):
        cases[f"edge_{d:+d}"] = a + zeros(window + d - 300) + a                 # pairs from window + d back: d = 1 straddles
    return cases


@functools.lru_cache(maxsize=None)
def window_chunks(window):
    """name -> (LZW stream, decoded bytes, (bytes, status) of the reference decoder)"""
    out = {}
    for name, raw in window_streams(window).items():
        s = tc.lzw_strip(raw)
        out[name] = (s, raw, dc.lzw_decode_strip(s, len(raw)))
    return out


def length_streams(window):
    """decoded lengths around the window and the flush block, and one that is no multiple of 16"""
    return {f"len_{n}": dc.values_strip(n, 7, seed=n) for n in (window - 1, window, window + 1, BLOCK - 1, BLOCK, BLOCK + 1, 1, 5003)}


def malformed_chunks():
    """name -> (stream, dst_len, mode): streams with a defined outcome other than 0 (or 0 without an EOI)"""
    good = tc.lzw_strip(dc.values_strip(40000, 5, seed=9))
    return {
        "truncated": (good[:len(good) // 2], 40000, 1),                          # status 1 after more than a window of output
        "truncated_far": (tc.lzw_strip(_rand(300, 21) + bytes(30000) + _rand(300, 21))[:-40], 30600, 1),
        "empty": (b"", 100, 1),
        "eoi_first": (dc.pack_codes([(256, 9), (257, 9)]), 100, 1),
        "eoi_early": (tc.lzw_strip(b"abcabcabc" * 50), 1000, 1),                 # status 2 with 450 bytes there
        "table_code_after_clear": (dc.pack_codes([(256, 9), (300, 9)]), 100, 1),
        "table_code_first": (dc.pack_codes([(258, 9), (65, 9)]), 100, 1),
        "code_above_next": (dc.pack_codes([(256, 9), (65, 9), (66, 9), (300, 9)]), 100, 1),
        "no_eoi_needed": (good[:-2], 39000, 1),                                  # status 0: dst_len bytes exist before the end
        "stored_short": (b"0123456789", 12, 0),                                  # stored: status 1, 10 bytes written
        "stored_long": (bytes(range(200)), 131, 0),
    }


def chunk_launch(chunks, slot_bytes=None, misalign=0):
    """The arrays of one launch from (stream, dst_len, mode) triples: (src, src_off, src_len, dst_len, mode, slot_bytes).  Streams lie
    in ``src`` in order with bytes of 0xFF between them, stream i at an offset that is (misalign + i) modulo 4."""
    parts, off, at = [], [], 0
    for i, (s, _, _) in enumerate(chunks):
        pad = (misalign + i - at) % 4
        parts.append(b"\xff" * pad + s)
        off.append(at + pad)
        at += pad + len(s)
    parts.append(b"\xff" * 3)
    longest = max(max(n for _, n, _ in chunks), 1)
    slot = slot_bytes or -(-longest // GUARD) * GUARD
    return (np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(off, np.int64), np.array([len(s) for s, _, _ in chunks], np.int32),
            np.array([n for _, n, _ in chunks], np.int32), np.array([m for _, _, m in chunks], np.int32), slot)


def reference_chunk(stream, dst_len, mode):
    """(bytes written to the slot's front, status) by the kernel's contract"""
    if mode == 0:
        return stream[:dst_len], 0 if len(stream) >= dst_len else 1
    return dc.lzw_decode_strip(stream, dst_len)


# ---------------------------------------------------------------------------------------------------------- chunks_to_planes
def unpredict(chunk, samples):
    """TIFF predictor 2 undone on a (rows, width * samples) uint8 chunk: per row and sample the running sum modulo 256"""
    rows = chunk.shape[0]
    return np.cumsum(chunk.reshape(rows, -1, samples), axis=1, dtype=np.uint8).reshape(rows, -1)


def unpredict_slow(chunk, samples):
    out = chunk.copy()
    for r in range(out.shape[0]):
        for k in range(samples, out.shape[1]):
            out[r, k] = (int(out[r, k]) + int(out[r, k - samples])) & 255
    return out


def predict(chunk, samples):
    """the writer's side: horizontal differencing of a (rows, width * samples) chunk"""
    out = chunk.copy()
    out[:, samples:] = chunk[:, samples:] - chunk[:, :-samples]
    return out


def planes_ref(slots, table, status, samples, predictor, planes):
    """flair_tiff_chunks_to_planes on the host: ``slots`` the decoded bytes of every chunk, ``planes`` (bands, H, W) written in place"""
    bands, H, W = planes.shape
    for raw, (x0, y0, width, rows, band0), st in zip(slots, table, status):
        if st != 0:
            continue
        chunk = np.frombuffer(raw, np.uint8)[:rows * width * samples].reshape(rows, width * samples)
        if predictor == 2:
            chunk = unpredict(chunk, samples)
        px = chunk.reshape(rows, width, samples)
        h, w = min(rows, H - y0), min(width, W - x0)     # edge tiles are clipped on the right and at the bottom
        if h > 0 and w > 0:
            planes[band0:band0 + samples, y0:y0 + h, x0:x0 + w] = px[:h, :w].transpose(2, 0, 1)
    return planes


def chunk_grid(H, W, bands, planar, cw, ch, tiled):
    """(n, 5) int32 {x0, y0, width, rows, band0} in TIFF chunk order: tiles are full size, the last strip is short"""
    rows = []
    for b in range(bands if planar == 2 else 1):
        for y0 in range(0, H, ch):
            for x0 in range(0, W, cw):
                rows.append((x0, y0, cw, ch if tiled else min(ch, H - y0), b))
    return np.array(rows, np.int32)


def chunk_bytes(raster, planar, x0, y0, width, rows, band0):
    """the decoded bytes of one chunk of a (bands, H, W) raster before any predictor: zeros outside the raster"""
    bands, H, W = raster.shape
    sel = raster if planar == 1 else raster[band0:band0 + 1]
    px = np.zeros((rows, width, sel.shape[0]), np.uint8)
    h, w = min(rows, H - y0), min(width, W - x0)
    px[:h, :w] = sel[:, y0:y0 + h, x0:x0 + w].transpose(1, 2, 0)
    return px.reshape(rows, -1)


# ---------------------------------------------------------------------------------------------------------------- whole files
def build_tiff(raster, tile=None, rows_per_strip=None, planar=1, compression=5, predictor=1, bigtiff=False, order="<", override=None,
               drop=(), offset_type=None, extra=None, mangle=None):
    """A TIFF of a (bands, H, W) uint8 raster framed on the host: ``tile`` = (width, length) or strips of ``rows_per_strip`` rows, any
    byte order.  ``override`` {tag: (type, values)} replaces entries, ``drop`` removes them, ``extra`` adds some, ``offset_type`` sets
    the type of the offset and count arrays, ``mangle(i, stream)`` rewrites chunk i's bytes: for the files a reader must refuse."""
    bands, H, W = raster.shape
    tiled = tile is not None
    cw, ch = tile if tiled else (W, rows_per_strip or H)
    if bands == 1:
        planar = 1
    samples = bands if planar == 1 else 1
    streams = []
    for x0, y0, width, rows, band0 in chunk_grid(H, W, bands, planar, cw, ch, tiled):
        chunk = chunk_bytes(raster, planar, x0, y0, width, rows, band0)
        if predictor == 2:
            chunk = predict(chunk, samples)
        s = chunk.tobytes()
        s = tc.lzw_strip(s) if compression == 5 else s
        streams.append(mangle(len(streams), s) if mangle else s)
    e = order
    hdr = 16 if bigtiff else 8
    offsets, at = [], hdr
    for s in streams:
        offsets.append(at)
        at += len(s) + len(s) % 2
    ot = offset_type or (16 if bigtiff else 4)
    entries = {256: (4, (W,)), 257: (4, (H,)), 258: (3, (8,) * bands), 259: (3, (compression,)), 262: (3, (2 if bands == 3 else 1,)),
               277: (3, (bands,)), 284: (3, (planar,)), 339: (3, (1,) * bands)}
    if predictor != 1:
        entries[317] = (3, (predictor,))
    if bands > 1 and bands != 3:
        entries[338] = (3, (0,) * (bands - 1))
    if tiled:
        entries.update({322: (4, (cw,)), 323: (4, (ch,)), 324: (ot, offsets), 325: (ot, [len(s) for s in streams])})
    else:
        entries.update({278: (4, (ch,)), 273: (ot, offsets), 279: (ot, [len(s) for s in streams])})
    entries.update(extra or {})
    entries.update(override or {})
    for tag in drop:
        del entries[tag]
    ifd = at + at % 2
    inline, esize, cfmt, ofmt = (8, 20, "Q", "Q") if bigtiff else (4, 12, "H", "I")
    tail_at = ifd + struct.calcsize(cfmt) + esize * len(entries) + inline
    head, tail = [struct.pack(e + cfmt, len(entries))], []
    for tag in sorted(entries):
        typ, vals = entries[tag]
        raw = struct.pack(f"{e}{len(vals)}{wc.TYPE_FMT[typ]}", *vals)
        if len(raw) <= inline:
            value = raw.ljust(inline, b"\0")
        else:
            value = struct.pack(e + ofmt, tail_at)
            tail.append(raw + b"\0" * (len(raw) % 2))
            tail_at += len(tail[-1])
        head.append(struct.pack(f"{e}HH{ofmt}", tag, typ, len(vals)) + value)
    head.append(b"\0" * inline)
    mark = b"II" if e == "<" else b"MM"
    header = struct.pack(e + "2sHHHQ", mark, 43, 8, 0, ifd) if bigtiff else struct.pack(e + "2sHI", mark, 42, ifd)
    body = b"".join(s + b"\0" * (len(s) % 2) for s in streams)
    return header + body + b"\0" * (ifd - at) + b"".join(head + tail)


def pil_file(img, **kw):
    return dc.pil_file(img, compression="tiff_lzw", **kw)


@functools.lru_cache(maxsize=None)
def accepted_files():
    """name -> (file bytes, the (bands, H, W) pixels a reader must return): every family raster_layout accepts"""
    files = {}
    r5 = wc.labels(5, 40, 56, seed=31)
    for il in ("band", "pixel"):
        for big in (False, True):
            data = wc.frame(40, 56, 5, 16, il, wc.ref_streams(r5, 16, il), bigtiff=big)
            files[f"framed_{il}_{'big' if big else 'classic'}"] = (data, wc.read_file(data))
    grey = dc.small_image(70, 45)
    rgb = np.ascontiguousarray(wc.labels(3, 70, 45, seed=32).transpose(1, 2, 0))
    for name, img in (("L", grey), ("RGB", rgb)):
        for pred in (False, True):
            data = pil_file(img, **({"tiffinfo": {317: 2}} if pred else {}))
            files[f"pil_{name}{'_pred2' if pred else ''}"] = (data, wc.pil_read(data)[1])
    odd = wc.labels(5, 37, 53, seed=33)
    smooth = (np.add.outer(np.arange(37), np.arange(53))[None] * np.arange(1, 6)[:, None, None] // 3).astype(np.uint8)   # gradients
    built = {
        "mm_classic_tiled": dict(tile=(16, 16), planar=2, order=">"),
        "mm_big_strips_pixel": dict(rows_per_strip=7, planar=1, order=">", bigtiff=True),
        "strips_band_pred2": dict(rows_per_strip=7, planar=2, predictor=2),
        "strips_pixel_pred2": dict(rows_per_strip=1, planar=1, predictor=2),
        "one_strip": dict(rows_per_strip=None, planar=1),
        "tiles_16x32_pixel_pred2": dict(tile=(16, 32), planar=1, predictor=2),
        "tiles_32x16_band": dict(tile=(32, 16), planar=2),
        "stored_tiles": dict(tile=(16, 16), planar=1, compression=1),
        "stored_strips_band": dict(rows_per_strip=5, planar=2, compression=1),
        "short_offsets": dict(rows_per_strip=3, planar=1, offset_type=3),
    }
    for name, kw in built.items():
        raster = smooth if "pred2" in name else odd
        files[name] = (build_tiff(raster, **kw), raster)
    return files


def refused_files():
    """name -> (file bytes, a word the refusal must contain)"""
    r = wc.labels(2, 37, 53, seed=34)
    tiled = dict(tile=(16, 16), planar=2)
    good = build_tiff(r, **tiled)
    assert good[:2] == b"II"
    (ifd,) = struct.unpack_from("<I", good, 4)
    lsb = lambda i, s: b"\x00\x01" + s[2:] if i == 3 else s   # noqa: E731
    return {
        "deflate": (build_tiff(r, **tiled, override={259: (3, (8,))}), "Compression"),
        "jpeg": (build_tiff(r, **tiled, override={259: (3, (7,))}), "Compression"),
        "bits_16": (build_tiff(r, **tiled, override={258: (3, (16, 16))}), "BitsPerSample"),
        "bits_missing": (build_tiff(r, **tiled, drop=(258,)), "BitsPerSample"),
        "bits_one_value": (build_tiff(r, **tiled, override={258: (3, (8,))}), "BitsPerSample"),
        "float_samples": (build_tiff(r, **tiled, override={339: (3, (3, 3))}), "SampleFormat"),
        "predictor_3": (build_tiff(r, **tiled, override={317: (3, (3,))}), "Predictor"),
        "predictor_2_stored": (build_tiff(r, **tiled, compression=1, extra={317: (3, (2,))}), "Predictor"),
        "fill_order_2": (build_tiff(r, **tiled, extra={266: (3, (2,))}), "FillOrder"),
        "orientation_3": (build_tiff(r, **tiled, extra={274: (3, (3,))}), "Orientation"),
        "planar_3": (build_tiff(r, **tiled, override={284: (3, (3,))}), "PlanarConfiguration"),
        "tile_width_24": (build_tiff(r, **tiled, override={322: (4, (24,))}), "TileWidth"),
        "tile_length_missing": (build_tiff(r, **tiled, drop=(323,)), "TileLength"),
        "rows_per_strip_0": (build_tiff(r, rows_per_strip=5, override={278: (4, (0,))}), "RowsPerStrip"),
        "reduced_subfile": (build_tiff(r, **tiled, extra={254: (4, (1,))}), "NewSubfileType"),
        "width_0": (build_tiff(r, **tiled, override={256: (4, (0,))}), "ImageWidth"),
        "length_missing": (build_tiff(r, **tiled, drop=(257,)), "ImageLength"),
        "offsets_too_few": (build_tiff(r, **tiled, override={324: (4, tuple(range(8, 8 + 23)))}), "TileOffsets"),
        "counts_too_many": (build_tiff(r, **tiled, override={325: (4, (10,) * 25)}), "TileByteCounts"),
        "offsets_missing": (build_tiff(r, rows_per_strip=5, drop=(273,)), "StripOffsets"),
        "offsets_as_bytes": (build_tiff(r, rows_per_strip=37, offset_type=1, mangle=lambda i, s: s[:200]), "StripOffsets"),
        "offset_outside": (build_tiff(r, **tiled, override={324: (4, (8,) * 23 + (len(good),))}), "TileOffsets"),
        "count_outside": (build_tiff(r, rows_per_strip=37, override={279: (4, (1 << 20,))}), "StripOffsets"),
        "lsb_first_lzw": (build_tiff(r, **tiled, mangle=lsb), "Compression"),
        "cut_in_arrays": (good[:-5], "TileByteCounts"),
        "cut_in_ifd": (good[:ifd + 20], "IFD"),
        "cut_in_header": (good[:6], "TIFF"),
        "cut_in_data": (good[:ifd // 2], "IFD"),
        "not_a_tiff": (b"\x89PNG" + good[4:], "TIFF"),
        "magic_44": (good[:2] + struct.pack("<H", 44) + good[4:], "TIFF"),
    }
