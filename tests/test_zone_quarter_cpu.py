"""The float64 restatement of the x4 bilinear resize (align_corners=False) that tests/test_gpu_zone_quarter.py feeds to the
stitching restatement of tests/test_zone_stitch_cpu.py: pinned here against torch.nn.functional.interpolate in float64, and
shown to be exact in fp32 on the integer logits the bit-exact GPU tests use."""
import numpy as np
import pytest
import torch


def _axis(n_out):
    """source coordinate (o + 0.5) / 4 - 0.5 clamped at 0; lower index, upper index clamped to the last, upper weight"""
    n_in = n_out // 4
    s = np.maximum((np.arange(n_out, dtype=np.float64) + 0.5) / 4.0 - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, s - i0


def upsample4_np(x):
    """(..., h, w) -> (..., 4h, 4w) float64"""
    x = np.asarray(x, dtype=np.float64)
    h, w = x.shape[-2:]
    y0, y1, ly = _axis(4 * h)
    x0, x1, lx = _axis(4 * w)
    ly = ly[:, None]
    top = (1.0 - lx) * x[..., y0, :][..., :, x0] + lx * x[..., y0, :][..., :, x1]
    bot = (1.0 - lx) * x[..., y1, :][..., :, x0] + lx * x[..., y1, :][..., :, x1]
    return (1.0 - ly) * top + ly * bot


def _interp(x):
    return torch.nn.functional.interpolate(x, scale_factor=4, mode="bilinear", align_corners=False)


@pytest.mark.parametrize("h,w", [(2, 2), (16, 16), (16, 24)])
def test_restatement_is_torch_interpolate_in_float64(h, w):
    x = np.random.default_rng(h * 100 + w).normal(0, 3, size=(2, 3, h, w))
    want = _interp(torch.from_numpy(x)).numpy()
    got = upsample4_np(x)
    assert got.shape == (2, 3, 4 * h, 4 * w) and got.dtype == np.float64
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("h", [2, 16, 32])
def test_integer_logits_interpolate_exactly_in_fp32(h):
    """weights are multiples of 1/8 per axis, so integers in [-8, 8] give multiples of 1/64 below 2^4: every product and sum
    is exact in fp32 however it is contracted"""
    x = np.random.default_rng(h).integers(-8, 9, size=(1, 5, h, h)).astype(np.float32)
    f32 = _interp(torch.from_numpy(x)).numpy()
    f64 = upsample4_np(x)
    assert f32.dtype == np.float32 and np.array_equal(f32.astype(np.float64), f64)
    assert np.array_equal(f64 * 64, np.round(f64 * 64))


def test_a_2x2_source_clamps_at_both_ends():
    """S = 8: outputs 0-1 have their coordinate clamped at 0, outputs 6-7 their upper index clamped to the last cell"""
    y0, y1, ly = _axis(8)
    assert list(y0) == [0, 0, 0, 0, 0, 0, 1, 1] and list(y1) == [1, 1, 1, 1, 1, 1, 1, 1]
    assert ly[0] == 0 and ly[1] == 0 and list(ly[2:6]) == [0.125, 0.375, 0.625, 0.875]


def test_detect_convert_rejects_an_upsample_it_does_not_have():
    from flair_amd.zone_detect import detect_convert
    with pytest.raises(ValueError, match="upsample"):
        detect_convert(torch.zeros(1, 3, 4, 4), 0, "argmax", upsample=2)
