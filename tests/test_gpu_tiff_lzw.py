"""csrc/tiff_lzw.hip through the C ABI, flair_amd.ops.tiff_lzw_encode and predictionwriter(encode="device"): the kernel's bytes equal
the reference encoder of tiff_lzw_cases strip for strip, stay inside their slots, and decode with PIL / libtiff to the input."""
import io

import numpy as np
import pytest
import torch

import tiff_lzw_cases as tc

pytestmark = pytest.mark.gpu


def _encode(dev, imgs, R, extra_slots=0, fill=None):
    """(B, H, W) uint8 numpy -> per tile, per strip: the bytes of its slot up to its count; and the whole output buffer"""
    from flair_amd import _lib as L
    lib = L.lib()
    B, H, W = imgs.shape
    nstrips = -(-H // R)
    slot = lib.flair_tiff_lzw_slot_bytes(R, W)
    assert slot == tc.slot_bytes(R, W)
    x = torch.from_numpy(np.ascontiguousarray(imgs)).to(dev)
    out = torch.empty((B * nstrips + extra_slots) * slot, dtype=torch.uint8, device=dev)
    if fill is not None:
        out.fill_(fill)
    counts = torch.full((B * nstrips,), -1, dtype=torch.int32, device=dev)
    L.check(lib.flair_tiff_lzw_encode(L.ptr(x), B, H, W, R, L.ptr(out), slot, L.ptr(counts), L.stream()), "flair_tiff_lzw_encode")
    out_h = out.cpu().numpy()
    counts_h = counts.cpu().numpy().reshape(B, nstrips)
    strips = [[out_h[(b * nstrips + s) * slot:][:counts_h[b, s]].tobytes() for s in range(nstrips)] for b in range(B)]
    return strips, counts_h, out_h, slot


def _assert_equals_reference(imgs, R, strips, counts):
    for b, img in enumerate(imgs):
        want = tc.ref_strips(img, R)
        assert [len(w) for w in want] == counts[b].tolist(), (b, counts[b].tolist())
        for s, w in enumerate(want):
            assert strips[b][s] == w, f"tile {b} strip {s}: first difference at byte " \
                f"{next(i for i, (p, q) in enumerate(zip(strips[b][s], w)) if p != q)} of {len(w)}"


def _case(name):
    rng = np.random.default_rng(21)
    if name == "a":   # odd width, unaligned strips, a short last strip, several tiles
        return rng.integers(0, 19, (3, 40, 37)).astype(np.uint8), 16
    if name == "b":   # long matches
        return np.stack([np.full((64, 64), 5, np.uint8), np.tile(np.arange(64, dtype=np.uint8) * 4 + 3, (64, 1))]), 8
    if name == "b256":   # the 0..255 ramp of every row, 256 wide
        return np.stack([np.full((64, 256), 5, np.uint8), np.tile(np.arange(256, dtype=np.uint8), (64, 1))]), 8
    if name == "c":
        return np.array([[[77]]], np.uint8), 1
    if name == "d":   # one 8 KB strip across all three width switches and the table reset
        return rng.integers(0, 256, (1, 16, 512)).astype(np.uint8), 16
    raise KeyError(name)


@pytest.mark.parametrize("name", ["a", "b", "b256", "c", "d"])
def test_bytes_equal_the_reference_encoder(dev, name):
    imgs, R = _case(name)
    strips, counts, _, _ = _encode(dev, imgs, R)
    _assert_equals_reference(imgs, R, strips, counts)


def test_boundary_lengths(dev):
    """strip lengths whose end-of-strip step lands on a width switch (512 / 1024 / 2048) or on the reset threshold (4094), their
    neighbours, and one past the reset; computed with the reference encoder's own counter"""
    row = tc.boundary_row()
    exact, lengths = tc.boundary_lengths(row)
    assert len(exact) == 4 and exact == sorted(exact) and 5999 in lengths and len(lengths) == 13
    for L in lengths:
        imgs = row[:L].reshape(1, 1, L)
        strips, counts, _, _ = _encode(dev, imgs, 1)
        _assert_equals_reference(imgs, 1, strips, counts)


def test_nothing_is_written_outside_a_slot(dev):
    imgs, R = _case("a")
    strips, counts, out, slot = _encode(dev, imgs, R, extra_slots=1, fill=0xA5)
    n = imgs.shape[0] * -(-imgs.shape[1] // R)
    assert out.size == (n + 1) * slot and (out[n * slot:] == 0xA5).all()
    _assert_equals_reference(imgs, R, strips, counts)   # so no neighbour overwrote a strip either
    # a store may be padded past the count, to the next 32-bit word at most
    for i, c in enumerate(counts.reshape(-1)):
        assert (out[i * slot + (c + 3) // 4 * 4:(i + 1) * slot] == 0xA5).all(), i


@pytest.mark.parametrize("name", ["a", "b", "d"])
def test_files_from_kernel_output_open_with_pil(dev, name):
    from PIL import Image
    from flair_amd.writer import tiff_lzw_file
    imgs, R = _case(name)
    strips, _, _, _ = _encode(dev, imgs, R)
    for b, img in enumerate(imgs):
        im = Image.open(io.BytesIO(tiff_lzw_file(img.shape[0], img.shape[1], R, strips[b])))
        assert im.mode == "L" and np.array_equal(np.asarray(im), img)


def test_ops_wrapper_default_strips(dev):
    from flair_amd import ops
    imgs = np.random.default_rng(4).integers(0, 19, (2, 40, 512)).astype(np.uint8)
    out, counts, slot, R = ops.tiff_lzw_encode(torch.from_numpy(imgs).to(dev))
    assert R == 16 and slot == tc.slot_bytes(16, 512) and out.shape == (2, 3, slot) and counts.shape == (2, 3)
    out, counts = out.cpu().numpy(), counts.cpu().numpy()
    for b in range(2):
        assert [out[b, s, :counts[b, s]].tobytes() for s in range(3)] == tc.ref_strips(imgs[b], 16)
    with pytest.raises(ValueError):
        ops.tiff_lzw_encode(torch.from_numpy(imgs).to(dev), rows_per_strip=0)


def test_writer_device_mode(dev, tmp_path):
    from PIL import Image
    from flair_amd.writer import predictionwriter
    rng = np.random.default_rng(9)
    preds = rng.integers(0, 19, (7, 64, 64))
    preds[1] = 3
    cfg = {"georeferencing_output": False}
    dirs = {}
    for mode in ("device", "host"):
        dirs[mode] = tmp_path / mode
        w = predictionwriter(cfg, str(dirs[mode]), "batch", encode=mode)
        for i in (0, 2, 4, 6):
            j = min(i + 2, 7)   # three batches of 2, a last batch of 1
            batch = {"preds": torch.from_numpy(preds[i:j]).to(dev), "id": [f"/data/x/img/IMG_{k:06d}.tif" for k in range(i, j)]}
            w.on_predict_batch_end(None, None, batch, batch, i // 2)
        w.on_predict_epoch_end(None, None)
        if mode == "device":
            with pytest.raises(RuntimeError):
                w.write_on_batch_end(None, None, {"preds": torch.from_numpy(preds[:1]), "id": ["IMG_x.tif"]}, None, None, 0, 0)
        w.on_predict_end(None, None)
        assert w._worker is None
    assert sorted(p.name for p in dirs["device"].iterdir()) == sorted(p.name for p in dirs["host"].iterdir()) \
        == [f"PRED_IMG_{k:06d}.tif" for k in range(7)]
    for k in range(7):
        got = Image.open(dirs["device"] / f"PRED_IMG_{k:06d}.tif")
        assert got.mode == "L" and np.array_equal(np.asarray(got), preds[k].astype(np.uint8))
        assert np.array_equal(np.asarray(got), np.asarray(Image.open(dirs["host"] / f"PRED_IMG_{k:06d}.tif")))
    with pytest.raises(RuntimeError):
        predictionwriter({"georeferencing_output": True}, str(tmp_path / "geo"), "batch", encode="device").write_on_batch_end(
            None, None, batch, None, batch, 0, 0)


def test_argument_errors_launch_nothing(dev):
    from flair_amd import _lib as L
    lib = L.lib()
    H, W, R = 16, 32, 8
    slot = lib.flair_tiff_lzw_slot_bytes(R, W)
    x = torch.zeros(1, H, W, dtype=torch.uint8, device=dev)
    out = torch.full((2 * slot,), 0xA5, dtype=torch.uint8, device=dev)
    counts = torch.full((2,), -1, dtype=torch.int32, device=dev)
    px, po, pc, st = L.ptr(x), L.ptr(out), L.ptr(counts), L.stream()
    assert lib.flair_tiff_lzw_encode(px, 1, H, W, 0, po, slot, pc, st) < 0
    assert lib.flair_tiff_lzw_encode(px, 1, H, W, -3, po, slot, pc, st) < 0
    assert lib.flair_tiff_lzw_encode(px, 1, H, W, R, po, slot - 16, pc, st) < 0
    assert lib.flair_tiff_lzw_encode(px, 1, H, W, R, po, slot - 1, pc, st) < 0
    assert lib.flair_tiff_lzw_encode(None, 1, H, W, R, po, slot, pc, st) < 0
    assert lib.flair_tiff_lzw_encode(px, 1, H, W, R, None, slot, pc, st) < 0
    assert lib.flair_tiff_lzw_encode(px, 1, H, W, R, po, slot, None, st) < 0
    assert lib.flair_tiff_lzw_encode(px, 0, H, W, R, po, slot, pc, st) < 0
    assert lib.flair_tiff_lzw_encode(px, 1, H, W, R, po + 4, slot, pc, st) < 0   # slots are written as aligned words
    torch.cuda.synchronize()
    assert (out.cpu() == 0xA5).all() and (counts.cpu() == -1).all()
    assert lib.flair_tiff_lzw_encode(px, 1, H, W, R, po, slot, pc, st) == 0
    assert (counts.cpu() > 0).all()
