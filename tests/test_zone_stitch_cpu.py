"""zone_detect's comparison pipeline on the host (no device): gen_param_combination against src/zone_detect/utils.py:110-166,
the combination config ZoneDetector accepts, and the float64 numpy restatement of the overlap stitching modes that
tests/test_gpu_zone_stitch.py compares the device against (its semantics: DESIGN §8, "overlap stitching").

Restatement (every window of tile_grid in job order contributes its margin-cropped centre
[x0+m, x0+S-m) x [y0+m, y0+S-m), clipped to the raster; p = softmax over classes of the window's logits):
    'average'          sum(p) / n over the covering windows
    'average_weights'  sum(w p) / sum(w), w = patch_weights(S, 0.5, 'exp') at the pixel's position inside the window
    'max'              (class, probability) of the covering window with the largest max probability; a later window wins
                       unless the held probability is strictly greater (compare.py:135-136, on the confidence band)
    output             [first argmax, its probability] (convert 'argmax'); pixels no core reaches stay 0.
"""
import numpy as np
import pytest

from flair_amd import zone_detect as zd


def softmax64(lg):
    x = np.asarray(lg, dtype=np.float64)
    e = np.exp(x - x.max(axis=0, keepdims=True))
    return e / e.sum(axis=0, keepdims=True)


def _top2(p):
    s = np.sort(p, axis=0)
    return s[-1] - s[-2]


def _core(x0, y0, S, m, H, W):
    return max(y0 + m, 0), min(y0 + S - m, H), max(x0 + m, 0), min(x0 + S - m, W)


def stitch_np(logits, grid, H, W, S, m, method):
    """logits (N, C, S, S) of the N windows of ``grid`` (tile_grid rows, job order).  Returns (out (2, H, W) float64,
    gap (H, W)): gap is how far the class decision is from a tie (top-2 probability gap of the blended probabilities; for
    'max' also the smallest difference of the compared window probabilities), +inf where no window reached the pixel."""
    N, C = logits.shape[:2]
    out = np.zeros((2, H, W))
    gap = np.full((H, W), np.inf)
    if method == "max":
        for n in range(N):
            x0, y0 = int(grid[n, 0]), int(grid[n, 1])
            ya, yb, xa, xb = _core(x0, y0, S, m, H, W)
            p = softmax64(logits[n])[:, ya - y0:yb - y0, xa - x0:xb - x0]
            cls, pb, g2 = p.argmax(0), p.max(0), _top2(p)
            past = out[1, ya:yb, xa:xb]
            keep = past > pb
            g = gap[ya:yb, xa:xb]
            gap[ya:yb, xa:xb] = np.minimum(np.where(keep, g, g2), np.abs(past - pb))
            out[0, ya:yb, xa:xb] = np.where(keep, out[0, ya:yb, xa:xb], cls)
            out[1, ya:yb, xa:xb] = np.where(keep, past, pb)
        return out, gap
    if method not in ("average", "average_weights"):
        raise ValueError(method)
    w = zd.patch_weights(S, 0.5, "exp") if method == "average_weights" else np.ones((S, S))
    acc = np.zeros((C, H, W))
    ws = np.zeros((H, W))
    for n in range(N):
        x0, y0 = int(grid[n, 0]), int(grid[n, 1])
        ya, yb, xa, xb = _core(x0, y0, S, m, H, W)
        wc = w[ya - y0:yb - y0, xa - x0:xb - x0]
        acc[:, ya:yb, xa:xb] += wc * softmax64(logits[n])[:, ya - y0:yb - y0, xa - x0:xb - x0]
        ws[ya:yb, xa:xb] += wc
    cov = ws > 0
    pbar = acc[:, cov] / ws[cov]
    out[0][cov] = pbar.argmax(0)
    out[1][cov] = pbar.max(0)
    gap[cov] = _top2(pbar)
    return out, gap


def exact_np(logits, grid, H, W, S, m, gap_out=None):
    """Exact clipping (compare.py:69-82): each window writes the part of its core it owns (tile_grid columns 2-5).
    gap_out (H, W), optional: receives the owning window's top-2 probability gap."""
    out = np.zeros((2, H, W))
    for n in range(logits.shape[0]):
        x0, y0, wx0, wx1, wy0, wy1 = (int(v) for v in grid[n])
        p = softmax64(logits[n])[:, wy0 - y0:wy1 - y0, wx0 - x0:wx1 - x0]
        out[0, wy0:wy1, wx0:wx1] = p.argmax(0)
        out[1, wy0:wy1, wx0:wx1] = p.max(0)
        if gap_out is not None:
            gap_out[wy0:wy1, wx0:wx1] = _top2(p)
    return out


# ---------------------------------------------------------------------------------------------- gen_param_combination

BASE = {"img_pixels_detection": 512, "margin": 128, "output_type": "argmax"}


def test_gen_param_combination_default_is_one_exact_clipping_combination():
    # utils.py:116-134: no strategies -> padding ['no-padding'], tile size and margin of the config, ['exact-clipping'];
    # utils.py:153 get_stride without overlap_strat -> [S - 2m]
    got = zd.gen_param_combination(dict(BASE))
    assert got == [{"img_pixels_detection": 512, "margin": 128, "padding": "no-padding", "stitching": "exact-clipping", "stride": 256}]
    assert zd.method_name(got[0]) == "size=512_stride=256_margin=128_padding=no-padding_stitching=exact-clipping"  # main.py:302


def test_gen_param_combination_grid_fractional_margin_and_skips():
    cfg = dict(BASE, overlap_strat=True, strategies={
        "padding_overall": ["no-padding"],
        "tiling": {"enabled": True, "size_range": [256, 512], "stride_range": [0.25, 0.5]},
        "stitching": {"enabled": True, "margin": [0.25, 128, 0.5], "methods": ["average", "max"]}})
    got = zd.gen_param_combination(cfg)
    # utils.py:140-147: margin < 1 -> int(margin * size); size <= 2 * margin skipped (256 / 128 and every 0.5 margin);
    # utils.py:153 + tiles.py:4-15: overlap_strat -> strides int(f * size); loops padding > size > margin > stride > method
    want = []
    for S, m in ((256, 64), (512, 128), (512, 128)):
        for f in (0.25, 0.5):
            for meth in ("average", "max"):
                want.append({"img_pixels_detection": S, "margin": m, "padding": "no-padding", "stitching": meth, "stride": int(f * S)})
    assert got == want


def test_gen_param_combination_reads_methods_not_method():
    # utils.py:128: stitching_cfg.get("methods", ["exact-clipping"]); the shipped YAML writes `method:`, which is ignored
    cfg = dict(BASE, strategies={"stitching": {"enabled": True, "method": ["average", "max"]}})
    got = zd.gen_param_combination(cfg)
    assert [c["stitching"] for c in got] == ["exact-clipping"]
    cfg = dict(BASE, strategies={"stitching": {"enabled": False, "methods": ["average"]}})   # disabled: defaults (utils.py:130-131)
    assert [c["stitching"] for c in zd.gen_param_combination(cfg)] == ["exact-clipping"]
    cfg = dict(BASE, strategies={"stitching": {"enabled": True, "methods": ["average", "max"]}})
    got = zd.gen_param_combination(cfg)
    assert [c["stitching"] for c in got] == ["average", "max"] and {c["stride"] for c in got} == {256}


def test_gen_param_combination_does_not_mutate_config():
    cfg = dict(BASE, strategies={"stitching": {"enabled": True, "margin": [0.125], "methods": ["max"]}})
    zd.gen_param_combination(cfg)
    assert cfg["margin"] == 128 and cfg["img_pixels_detection"] == 512


# ---------------------------------------------------------------------------------------------- ZoneDetector config

def _cfg(**kw):
    c = {"img_pixels_detection": 64, "margin": 8, "output_type": "argmax", "n_classes": 13, "batch_size": 4, "channels": [1, 2, 3],
         "norma_task": [{"norm_type": "scaling"}]}
    c.update(kw)
    return c


def test_zone_detector_combination_config():
    d = zd.ZoneDetector(None, _cfg())
    assert (d.stitching, d.stride, d.blend) == ("exact-clipping", 48, None)
    d = zd.ZoneDetector(None, _cfg(stitching="average_weights", stride=16, padding="no-padding"))
    assert (d.stitching, d.stride, d.blend) == ("average_weights", 16, "average_weights")
    # a combination wins over overlap_strat (main.py:287-298 copies it into the config that still has the flag)
    d = zd.ZoneDetector(None, _cfg(overlap_strat=True, stitching="max", stride=24))
    assert (d.stride, d.blend) == (24, "max")
    # class_prob is stitched by exact clipping whatever the method (compare.py:67-68), with the combination's stride
    d = zd.ZoneDetector(None, _cfg(output_type="class_prob", stitching="average", stride=16))
    assert (d.stride, d.blend) == (16, None)
    d = zd.ZoneDetector(None, _cfg(stitching="exact-clipping", stride=20))
    assert (d.stride, d.blend) == (20, None)


def test_zone_detector_config_errors():
    with pytest.raises(NotImplementedError, match="gen_param_combination"):
        zd.ZoneDetector(None, _cfg(overlap_strat=True, strategies={"tiling": {"stride_range": [0.5]}}))
    with pytest.raises(ValueError, match="stride"):
        zd.ZoneDetector(None, _cfg(stitching="average"))
    with pytest.raises(ValueError, match="padding"):
        zd.ZoneDetector(None, _cfg(stitching="average", stride=16, padding="reflect"))
    with pytest.raises(ValueError, match="stitching"):
        zd.ZoneDetector(None, _cfg(stitching="median", stride=16))
    with pytest.raises(ValueError):
        zd.ZoneDetector(None, _cfg(stitching="max", stride=0))
    with pytest.raises(ValueError):
        zd.OverlapStitch("exact-clipping", np.zeros((1, 6), np.int32), 64, 8, 13, 64, 64, "cpu")


# ---------------------------------------------------------------------------------------------- the restatement itself

def test_weight_table_is_patch_weights_by_chebyshev_distance():
    for S in (64, 65, 512):
        t = zd.cheb_weight_table(S)
        assert t.dtype == np.float32 and t.shape == (S // 2 + 1,)
        c = S // 2
        ax = np.abs(np.arange(S) - c)
        d = np.maximum(ax[:, None], ax[None, :])
        np.testing.assert_array_equal(t[d], zd.patch_weights(S, 0.5, "exp").astype(np.float32))


@pytest.mark.parametrize("m", [0, 8])
def test_restatement_at_stride_k_is_exact_clipping(m):
    """Raster a multiple of K = S - 2m: the cores tile it, every pixel has one window, and every mode is exact clipping."""
    S, K = 64, 64 - 2 * m
    H, W = 2 * K, 3 * K
    grid = zd.tile_grid((W, H), S, m, K)
    lg = np.random.default_rng(m).normal(0, 3, size=(len(grid), 7, S, S)).astype(np.float32)
    want = exact_np(lg, grid, H, W, S, m)
    for method in ("average", "average_weights", "max"):
        got, gap = stitch_np(lg, grid, H, W, S, m, method)
        assert np.isfinite(gap).all()
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_allclose(got[1], want[1], rtol=0, atol=1e-15)


def test_restatement_overlap_properties():
    S, m, H, W = 32, 4, 50, 70
    grid = zd.tile_grid((W, H), S, m, 6)
    # identical windows everywhere (logits independent of the window): every mode gives that window's own result
    one = np.random.default_rng(0).normal(0, 2, size=(5, S, S)).astype(np.float32)
    same = np.broadcast_to(one, (len(grid), 5, S, S))
    avg, _ = stitch_np(same, grid, H, W, S, m, "average")
    mx, _ = stitch_np(same, grid, H, W, S, m, "max")
    const = np.broadcast_to(one[:, :1, :1], (len(grid), 5, S, S))
    a1, _ = stitch_np(const, grid, H, W, S, m, "average_weights")
    p = softmax64(one[:, 0, 0])
    np.testing.assert_allclose(a1[1], p.max(), atol=1e-12)
    assert (a1[0] == p.argmax()).all()
    assert np.all(mx[1] >= avg[1] - 1e-12)    # the max mode keeps the most confident window
    # stride > K leaves uncovered columns / rows at zero
    grid = zd.tile_grid((W, H), S, m, 30)
    lg = np.random.default_rng(1).normal(size=(len(grid), 5, S, S)).astype(np.float32)
    for method in ("average", "max"):
        out, gap = stitch_np(lg, grid, H, W, S, m, method)
        unc = np.isinf(gap)
        assert unc.any() and (out[:, unc] == 0).all() and (out[1, ~unc] > 0).all()
