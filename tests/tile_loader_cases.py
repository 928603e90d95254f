"""Shared cases of the tile loader tests (flair_amd/tile_loader.py, tiff_chunks_to_batch_kernel in csrc/tiff_read.hip): a numpy
restatement of flair_tiff_chunks_to_batch written from its contract in include/flair_hip.h, the table of one launch that reaches every
branch of the kernel, and batches of small tile and mask files of different layouts with the pixels they hold."""
import functools

import numpy as np

import raster_reader_cases as rc
import raster_writer_cases as wc
import tiff_lzw_decode_cases as dc

FILL = rc.FILL


def batch_ref(slots, table, status, planes, slot_bytes):
    """flair_tiff_chunks_to_batch on the host: ``slots`` the bytes of every slot, ``table`` (n, 8) rows {x0, y0, width, rows, plane0,
    samples, predictor, 0}, ``planes`` (n_planes, H, W) written in place"""
    P, H, W = planes.shape
    for raw, row, st in zip(slots, table, status):
        x0, y0, width, rows, plane0, samples, predictor = (int(v) for v in row[:7])
        if st != 0 or x0 < 0 or y0 < 0 or width < 1 or rows < 1 or samples < 1 or plane0 < 0 or plane0 + samples > P:
            continue
        if predictor not in (1, 2) or width * rows * samples > slot_bytes:
            continue
        px = np.frombuffer(raw, np.uint8)[:rows * width * samples].reshape(rows, width, samples)
        if predictor == 2:
            px = np.cumsum(px, axis=1, dtype=np.uint8)       # per chunk row and sample, modulo 256
        h, w = min(rows, H - y0), min(width, W - x0)         # what lies outside H x W is dropped
        if h > 0 and w > 0:
            planes[plane0:plane0 + samples, y0:y0 + h, x0:x0 + w] = px[:h, :w].transpose(2, 0, 1)
    return planes


KERNEL_SHAPE = (9, 37, 130)
KERNEL_SLOT = 3072
# {x0, y0, width, rows, plane0, samples, predictor}, status: widths 16, 53, 64, 65 and 130 (the carry of the scan crosses no, one and
# two trip boundaries), samples 1 and 3, both predictors, tiles clipped right and bottom, a failed chunk and every skip rule
KERNEL_ROWS = [
    ((0, 0, 130, 5, 0, 3, 2), 0),
    ((0, 5, 130, 4, 0, 3, 1), 0),
    ((0, 0, 64, 7, 3, 1, 2), 0),
    ((64, 0, 65, 7, 3, 1, 2), 0),
    ((0, 7, 53, 6, 3, 1, 1), 0),
    ((120, 30, 16, 16, 3, 1, 2), 0),          # clipped right and bottom
    ((96, 32, 64, 16, 4, 3, 2), 0),           # three samples, clipped right and bottom, ends in the last trip's first half
    ((65, 9, 65, 3, 7, 1, 2), 0),
    ((130 - 53, 20, 53, 10, 7, 1, 2), 0),     # ends on the last column
    ((16, 3, 16, 16, 8, 1, 2), 0),
    ((0, 20, 16, 4, 8, 1, 1), 2),             # status 2: skipped
    ((40, 20, 16, 4, 7, 3, 1), 0),            # plane0 + samples > n_planes
    ((-1, 0, 16, 4, 8, 1, 1), 0),
    ((0, -1, 16, 4, 8, 1, 1), 0),
    ((0, 0, 16, 0, 8, 1, 1), 0),
    ((0, 0, 0, 4, 8, 1, 1), 0),
    ((0, 0, 16, 4, 8, 0, 1), 0),
    ((0, 0, 16, 4, -1, 1, 1), 0),
    ((0, 0, 16, 4, 8, 1, 3), 0),
    ((0, 0, 16, 4, 8, 1, 0), 0),
    ((0, 0, 130, 37, 8, 1, 1), 0),            # 4 810 bytes > the slot
    ((48, 24, 16, 13, 8, 1, 1), 0),           # a good chunk after the skipped ones
]


def kernel_launch():
    """(scratch (n, KERNEL_SLOT) uint8 of noise, table (n, 8) int32, status int32, max_rows)"""
    n = len(KERNEL_ROWS)
    scratch = np.random.default_rng(11).integers(0, 256, (n, KERNEL_SLOT)).astype(np.uint8)
    table = np.zeros((n, 8), np.int32)
    table[:, :7] = [r for r, _ in KERNEL_ROWS]
    status = np.array([s for _, s in KERNEL_ROWS], np.int32)
    return scratch, table, status, int(table[:, 3].max())


# ------------------------------------------------------------------------------------------------------------------- tile files
IMAGE_LAYOUTS = {
    "tiled_band_lzw": dict(tile=(16, 16), planar=2),
    "strips_pixel_pred2": dict(rows_per_strip=7, planar=1, predictor=2),
    "stored_strips": dict(rows_per_strip=5, planar=1, compression=1),
    "mm_big_strips": dict(rows_per_strip=9, planar=2, order=">", bigtiff=True),
    "one_strip": dict(rows_per_strip=None, planar=1),
}


def tile_raster(i, H=32, W=32, bands=5):
    """label-like bytes for even i (LZW shrinks them), noise for odd i"""
    return wc.labels(bands, H, W, seed=100 + i) if i % 2 == 0 else wc.noise(bands, H, W, seed=100 + i)


def mask_raster(i, H=32, W=32):
    """raw labels 0 .. 24: 0 and the values above the class count are what read_msk turns into class 0"""
    return (wc.labels(1, H, W, seed=200 + i, k=25) % 25).astype(np.uint8)


def image_file(i, H=32, W=32, mangle=None):
    """(file bytes, (5, H, W) pixels) of tile i: the layouts of IMAGE_LAYOUTS in turn"""
    raster = tile_raster(i, H, W)
    kw = list(IMAGE_LAYOUTS.values())[i % len(IMAGE_LAYOUTS)]
    return rc.build_tiff(raster, mangle=mangle, **kw), raster


def mask_file(i, H=32, W=32):
    """(file bytes, (H, W) raw labels) of mask i: PIL's LZW strips, stored strips, LZW tiles of 16 x 16 in turn"""
    raw = mask_raster(i, H, W)
    if i % 3 == 0:
        return rc.pil_file(raw[0]), raw[0]
    if i % 3 == 1:
        return rc.build_tiff(raw, rows_per_strip=6, compression=1), raw[0]
    return rc.build_tiff(raw, tile=(16, 16)), raw[0]


@functools.lru_cache(maxsize=None)
def tile_set(n, H=32, W=32):
    """n tiles and masks: ([image bytes], (n, 5, H, W) pixels, [mask bytes], (n, H, W) raw labels)"""
    imgs, msks = [image_file(i, H, W) for i in range(n)], [mask_file(i, H, W) for i in range(n)]
    return [d for d, _ in imgs], np.stack([r for _, r in imgs]), [d for d, _ in msks], np.stack([r for _, r in msks])


def write_set(folder, n, H=32, W=32):
    """tile_set written to ``folder``: (image paths, pixels, mask paths, raw labels)"""
    img_bytes, img, msk_bytes, msk = tile_set(n, H, W)
    ip, mp = [], []
    for i in range(n):
        ip.append(str(folder / f"IMG_{i:06d}.tif"))
        mp.append(str(folder / f"MSK_{i:06d}.tif"))
        (folder / f"IMG_{i:06d}.tif").write_bytes(img_bytes[i])
        (folder / f"MSK_{i:06d}.tif").write_bytes(msk_bytes[i])
    return ip, img, mp, msk


def host_slots(data, layout):
    """the decoded bytes of every chunk of a file, through the reference decoder"""
    table, _, dst_len, _ = layout.decode_tables()
    slots = []
    for off, cnt, want in zip(layout.offsets, layout.counts, dst_len):
        raw = bytes(data[int(off):int(off + cnt)])
        px, status = (raw[:want], 0) if layout.compression == 1 else dc.lzw_decode_strip(raw, int(want))
        assert status == 0 and len(px) == want
        slots.append(px)
    return slots
