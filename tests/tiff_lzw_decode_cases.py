"""Shared cases of the TIFF LZW decode tests: the reference decoder (the specification of tiff_lzw_decode_kernel in csrc/tiff_lzw.hip:
its bytes and its status are what the kernel must produce), an encoder that clears its table in mid-stream as foreign writers may,
a packer of hand-made code sequences, and the strip tables of a launch with guard bytes around every region."""
import numpy as np

MAX_STRIP = 65536     # decoded bytes of an LZW strip the kernel takes
SMALL_STRIP = 16384   # ... in its small size class
GUARD = 64
FILL = 0xA5


def lzw_decode_strip(data: bytes, want: int):
    """(bytes, status) of one TIFF 6.0 LZW strip as libtiff reads it, decoded until ``want`` bytes are there.
    status 0: exactly ``want`` bytes; 1: the input ran out first; 2: EOI came first; 3: a non-literal code first after a clear or the
    start; 4: code > nxt, or code == nxt with a full table.  At 1 - 4 the bytes are what was decoded before the error."""
    nbits = 8 * len(data)
    word = int.from_bytes(data, "big")
    out = bytearray()
    table = {}
    nxt, width, pos, old = 258, 9, 0, None
    while True:
        if len(out) >= want:
            return bytes(out[:want]), 0
        if pos + width > nbits:
            return bytes(out), 1
        code = (word >> (nbits - pos - width)) & ((1 << width) - 1)
        pos += width
        if code == 256:
            table = {}
            nxt, width, old = 258, 9, None
            continue
        if code == 257:
            return bytes(out), 2
        if old is None:
            if code >= 256:
                return bytes(out), 3
            old = bytes([code])
            out += old
            continue
        if code < 256:
            s = bytes([code])
        elif code < nxt:
            s = table[code]
        elif code == nxt and nxt < 4096:
            s = old + old[:1]
        else:
            return bytes(out), 4
        out += s
        if nxt < 4096:
            table[nxt] = old + s[:1]
            nxt += 1
            if nxt in (511, 1023, 2047):
                width += 1
        old = s


def pack_codes(codes) -> bytes:
    """(code, width) pairs MSB first, the last byte zero-padded"""
    acc = nb = 0
    for code, width in codes:
        acc = (acc << width) | code
        nb += width
    pad = -nb % 8
    return (acc << pad).to_bytes((nb + pad) // 8, "big")


def lzw_strip_with_clears(data: bytes, every: int, reset_at: int = 4094) -> bytes:
    """tc.lzw_strip with a ClearCode and a fresh table after every ``every`` codes of data: a valid stream no libtiff writes.
    ``reset_at=None``: no reset at 4094 either; the table fills up (entry 4095 is the last) and the stream goes on in 12-bit codes."""
    out = bytearray()
    acc = nb = 0

    def put(code, width):
        nonlocal acc, nb
        acc = (acc << width) | code
        nb += width
        while nb >= 8:
            out.append((acc >> (nb - 8)) & 0xFF)
            nb -= 8
        acc &= (1 << nb) - 1

    def widen(nxt, width):
        return width + 1 if nxt in (512, 1024, 2048) else width

    table, nxt, width, prefix, emitted = {}, 258, 9, -1, 0
    put(256, width)
    for c in data:
        key = (prefix << 8) | c
        if prefix < 0:
            prefix = c
        elif key in table:
            prefix = table[key]
        else:
            put(prefix, width)
            emitted += 1
            if nxt < 4096:
                table[key] = nxt
                nxt += 1
                width = widen(nxt, width)
            if (reset_at is not None and nxt >= reset_at) or emitted % every == 0:
                put(256, width)
                table, nxt, width = {}, 258, 9
            prefix = c
    if prefix >= 0:
        put(prefix, width)
        nxt += 1
        width = widen(nxt, width)
    put(257, width)
    if nb:
        out.append((acc << (8 - nb)) & 0xFF)
    return bytes(out)


def strip_table(strips, guard=GUARD, misalign=0):
    """The arrays of one launch from (stream bytes, dst_len, mode) triples: (src uint8, src_off int64, src_len int32, dst_off int64,
    dst_len int32, mode int32, dst_bytes).  Streams lie back to back in ``src``; the regions of ``dst`` lie in order with ``guard``
    bytes before, between and after them (a region of a dst_len below 1 takes no room), ``misalign`` more before the first."""
    src = b"".join(s for s, _, _ in strips)
    src_off = np.cumsum([0] + [len(s) for s, _, _ in strips[:-1]]).astype(np.int64)
    src_len = np.array([len(s) for s, _, _ in strips], dtype=np.int32)
    dst_off, at = [], guard + misalign
    for _, n, _ in strips:
        dst_off.append(at)
        at += max(n, 0) + guard
    return (np.frombuffer(src, dtype=np.uint8).copy(), src_off, src_len, np.array(dst_off, dtype=np.int64),
            np.array([n for _, n, _ in strips], dtype=np.int32), np.array([m for _, _, m in strips], dtype=np.int32), at)


def guards_intact(dst, dst_off, dst_len, fill=FILL):
    """every byte of ``dst`` outside the regions still holds ``fill``"""
    outside = np.ones(dst.size, dtype=bool)
    for o, n in zip(dst_off, dst_len):
        if n > 0:
            outside[o:o + n] = False
    return bool((dst[outside] == fill).all())


def constant_strip(n=16384, value=7):
    return bytes([value]) * n


def values_strip(n, k, seed=11):
    return np.random.default_rng(seed).integers(0, k, n).astype(np.uint8).tobytes()


def pil_file(img, **kw) -> bytes:
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, format="TIFF", **kw)
    return buf.getvalue()


def small_image(H, W, k=19, seed=3):
    """cells of 8 pixels of k classes, 5 % redrawn: runs, like a mask"""
    rng = np.random.default_rng(seed)
    m = np.kron(rng.integers(0, k, (-(-H // 8), -(-W // 8))), np.ones((8, 8), dtype=np.int64))[:H, :W]
    salt = rng.random((H, W)) < 0.05
    m[salt] = rng.integers(0, k, int(salt.sum()))
    return np.ascontiguousarray(m.astype(np.uint8))
