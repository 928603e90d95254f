"""CPU side of the device LZW writer (no device needed): the reference encoder of tiff_lzw_cases and ``writer.tiff_lzw_file`` against
an independent decoder (PIL / libtiff), the size the strip layout costs, and the ``encode`` argument of ``predictionwriter``."""
import io

import numpy as np
import pytest
from PIL import Image

import tiff_lzw_cases as tc


def _images():
    rng = np.random.default_rng(11)
    return {"noise19_64x96": rng.integers(0, 19, (64, 96)).astype(np.uint8),
            "constant_64x64": np.full((64, 64), 7, np.uint8),
            "noise19_40x37": rng.integers(0, 19, (40, 37)).astype(np.uint8),
            "one_pixel": np.array([[200]], np.uint8)}


IMAGES = _images()


@pytest.mark.parametrize("rows", [8, 16, "H"])
@pytest.mark.parametrize("name", list(IMAGES))
def test_file_from_reference_strips_opens_with_pil(name, rows):
    from flair_amd.writer import tiff_lzw_file
    img = IMAGES[name]
    H, W = img.shape
    R = H if rows == "H" else rows
    strips = tc.ref_strips(img, R)
    assert len(strips) == -(-H // R)
    data = tiff_lzw_file(H, W, R, strips)
    im = Image.open(io.BytesIO(data))
    assert im.mode == "L" and im.size == (W, H)
    assert np.array_equal(np.asarray(im), img)
    tags = im.tag_v2
    assert sorted(tags) == [256, 257, 258, 259, 262, 273, 277, 278, 279, 284]
    assert (tags[256], tags[257], tags[259], tags[262], tags[277], tags[278], tags[284]) == (W, H, 5, 1, 1, R, 1)
    assert tuple(np.atleast_1d(tags[258])) == (8,)
    counts = tuple(np.atleast_1d(tags[279]))
    offsets = tuple(np.atleast_1d(tags[273]))
    assert counts == tuple(len(s) for s in strips)
    # header 8, IFD 2 + 10 * 12 + 4, then the two arrays unless the single strip's offset and count sit in the entries
    first = 134 + (8 * len(strips) if len(strips) > 1 else 0)
    assert offsets == tuple(first + sum(counts[:i]) for i in range(len(strips)))
    assert len(data) == first + sum(counts)


def test_strip_count_must_match():
    from flair_amd.writer import tiff_lzw_file
    with pytest.raises(ValueError):
        tiff_lzw_file(64, 64, 16, tc.ref_strips(IMAGES["constant_64x64"], 8))


def test_reference_stream_stays_inside_the_slot():
    """the longest streams there are: 256-value noise never matches, so every byte costs a code, and the table resets"""
    rng = np.random.default_rng(2)
    for R, W in ((16, 512), (1, 1), (3, 37), (1, 3836), (2, 3836)):
        n = R * W
        worst = len(tc.lzw_strip(rng.integers(0, 256, n).astype(np.uint8).tobytes()))
        assert worst <= tc.slot_bytes(R, W) and tc.slot_bytes(R, W) % 16 == 0


def test_size_cap_against_pil_on_the_smooth_mask():
    """A condition, not a measurement: 16-row strips restart the dictionary 32 times per tile, which may cost at most 25 % over PIL's
    own tiff_lzw file of the same mask (32 458 against 27 698 bytes, 1.17 x, with the reference encoder)."""
    from flair_amd.writer import tiff_lzw_file
    m = tc.smooth_mask()
    R = tc.default_rows_per_strip(512)
    assert R == 16
    ours = tiff_lzw_file(512, 512, R, tc.ref_strips(m, R))
    buf = io.BytesIO()
    Image.fromarray(m).save(buf, format="TIFF", compression="tiff_lzw")
    pil = buf.getvalue()
    print(f"strips: {len(ours)} B, PIL: {len(pil)} B, ratio {len(ours) / len(pil):.3f}")
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(ours))), m)
    assert len(ours) <= 1.25 * len(pil)


def test_encode_argument(tmp_path, monkeypatch):
    from flair_amd import writer
    cfg = {"georeferencing_output": False}
    monkeypatch.delenv("FLAIR_WRITER_ENCODE", raising=False)
    assert writer.ENCODE_DEFAULT == "host"
    assert writer.predictionwriter(cfg, str(tmp_path), "batch").encode == "host"
    assert writer.predictionwriter(cfg, str(tmp_path), "batch", encode=None).encode == "host"
    assert writer.predictionwriter(cfg, str(tmp_path), "batch", encode="device").encode == "device"
    with pytest.raises(ValueError):
        writer.predictionwriter(cfg, str(tmp_path), "batch", encode="bogus")
    monkeypatch.setenv("FLAIR_WRITER_ENCODE", "device")
    assert writer.predictionwriter(cfg, str(tmp_path), "batch").encode == "device"
    assert writer.predictionwriter(cfg, str(tmp_path), "batch", encode="host").encode == "host"
    monkeypatch.setenv("FLAIR_WRITER_ENCODE", "gpu")
    with pytest.raises(ValueError):
        writer.predictionwriter(cfg, str(tmp_path), "batch")
    monkeypatch.delenv("FLAIR_WRITER_ENCODE")
    monkeypatch.setattr(writer, "ENCODE_DEFAULT", "device")
    assert writer.predictionwriter(cfg, str(tmp_path), "batch").encode == "device"


def test_slot_bytes_agree_between_python_and_c():
    from flair_amd import ops
    for R, W in ((16, 512), (1, 1), (8, 37), (1, 6000), (64, 64), (512, 512)):
        assert ops.tiff_lzw_slot_bytes(R, W) == tc.slot_bytes(R, W)
    assert ops.tiff_lzw_slot_bytes(0, 512) < 0 and ops.tiff_lzw_slot_bytes(16, 0) < 0


def test_host_tensor_is_refused():
    import torch
    from flair_amd import ops
    from flair_amd._lib import FlairHipError
    with pytest.raises(FlairHipError):
        ops.tiff_lzw_encode(torch.zeros(1, 8, 8, dtype=torch.uint8))
    with pytest.raises(FlairHipError):
        ops.tiff_lzw_encode(torch.zeros(1, 8, 8, dtype=torch.int64))
