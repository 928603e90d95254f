"""Shared cases of the TIFF LZW tests: the reference encoder (the specification of csrc/tiff_lzw.hip: its bytes are what the kernel
must write), strip splitting, the seeded masks and the strip lengths that sit on the encoder's switches."""
import numpy as np


def lzw_strip(data: bytes, trace=None) -> bytes:
    """TIFF 6.0 LZW of one strip as libtiff writes it.  ``trace``, a list, receives after every input byte the next free code after
    the final code of the strip that ends with that byte (the encoder's own counter, as its end-of-strip step leaves it)."""
    out = bytearray(); acc = 0; nb = 0

    def put(code, width):
        nonlocal acc, nb
        acc = (acc << width) | code; nb += width
        while nb >= 8:
            out.append((acc >> (nb - 8)) & 0xFF); nb -= 8
        acc &= (1 << nb) - 1

    def widen(nxt, width):
        return width + 1 if nxt in (512, 1024, 2048) else width

    table = {}; nxt = 258; width = 9; prefix = -1
    put(256, width)
    for c in data:
        key = (prefix << 8) | c
        if prefix < 0:
            prefix = c
        elif key in table:
            prefix = table[key]
        else:
            put(prefix, width)
            table[key] = nxt; nxt += 1; width = widen(nxt, width)
            if nxt >= 4094:
                put(256, width); table = {}; nxt = 258; width = 9
            prefix = c
        if trace is not None:
            trace.append(nxt + 1)   # what the end-of-strip step below would make of nxt, were this the last byte
    if prefix >= 0:
        put(prefix, width); nxt += 1; width = widen(nxt, width)
    put(257, width)
    if nb: out.append((acc << (8 - nb)) & 0xFF)
    return bytes(out)


def default_rows_per_strip(W):
    return max(1, 8192 // W)


def slot_bytes(rows_per_strip, W):
    """the issue's formula, restated on the host: align16(ceil(1.5 * (n + n // 3836 + 4)))"""
    n = rows_per_strip * W
    codes = n + n // 3836 + 4
    return -(-((3 * codes + 1) // 2) // 16) * 16


def ref_strips(img, rows_per_strip):
    """reference streams of one (H, W) uint8 image, strip by strip"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    return [lzw_strip(img[r:r + rows_per_strip].tobytes()) for r in range(0, img.shape[0], rows_per_strip)]


def smooth_mask():
    """512 x 512: 32-pixel class cells of 19 classes, 2 % of the pixels redrawn"""
    rng = np.random.default_rng(0)
    m = np.kron(rng.integers(0, 19, (17, 17)), np.ones((32, 32), dtype=np.int64))[:512, :512]
    salt = rng.random((512, 512)) < 0.02
    m[salt] = rng.integers(0, 19, int(salt.sum()))
    return m.astype(np.uint8)


def noise_mask():
    return np.random.default_rng(0).integers(0, 19, (512, 512)).astype(np.uint8)


def boundary_row():
    return np.random.default_rng(5).integers(0, 256, 6000).astype(np.uint8)


def boundary_lengths(row):
    """Lengths L of row[:L] at which the next free code after the final code is exactly 512, 1024, 2048 and 4094 (the first such L
    each), found with the reference encoder's own counter; with L - 1 and L + 1 of each, and 5999."""
    tr = []
    lzw_strip(row.tobytes(), tr)
    exact = [tr.index(k) + 1 for k in (512, 1024, 2048, 4094)]
    return exact, sorted({L + d for L in exact for d in (-1, 0, 1)} | {5999})
