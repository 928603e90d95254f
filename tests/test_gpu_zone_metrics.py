"""zone_detect metrics on the device (csrc/zone_metrics.hip through flair_amd.zone_metrics and ZoneDetector.run(raster, truth))
against numpy / scipy restatements and tests/golden/zone_metrics_reference.* (the reference's own functions).  Counts are
integers: every matrix is compared bit for bit."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MEANS = [105.08, 110.87, 101.82, 106.38, 53.26]
STDS = [52.17, 45.38, 44, 39.69, 79.3]
METHODS = ("exact-clipping", "average", "average_weights", "max")
_W0 = {15, 16, 17, 19}   # weight-0 classes of configs/config_detect_compare_metrics.yaml


def _classes(C):
    return {c: [0 if c in _W0 else 1, f"class {c}"] for c in range(1, C + 1)}


def _confmat_np(truth_u8, pred, C):
    t = (np.asarray(truth_u8).astype(np.int64) - 1) % 256
    p = np.asarray(pred).astype(np.int64)
    ok = (t < C) & (p >= 0) & (p < C)
    return np.bincount(t[ok] * C + p[ok], minlength=C * C).reshape(C, C)


def _truth(rng, H, W, C):
    t = rng.integers(0, C + 1, size=(H, W)).astype(np.uint8)   # 0 = no data, dropped from the matrices
    t[: H // 5, : W // 3] = 0
    return t


def _window_cms(truth, cls, grid, S, m, C):
    """host matrices of each window's (K, K) class map against the truth over its core"""
    K = S - 2 * m
    out = []
    for b, (x0, y0) in enumerate(grid[:, :2]):
        cx, cy = x0 + m, y0 + m
        out.append(_confmat_np(truth[cy:cy + K, cx:cx + K], cls[b], C))
    return np.stack(out)


def _launch(fn, *args):
    from flair_amd import _lib as L
    L.check(getattr(L.lib(), fn)(*args, L.stream()), fn)


@pytest.mark.parametrize("C", [13, 19])
@pytest.mark.parametrize("m", [0, 8])
@pytest.mark.parametrize("dstride", [-8, 0, 8])
def test_window_confmats_three_sources(dev, C, m, dstride):
    """(a) u8 class tiles, (b) fp32 logits (the class flair_detect_stitch writes), (c) the finished fp32 raster; 150 x 190 is no
    multiple of any stride, so the last column and row of windows are pulled back"""
    from flair_amd import _lib as L
    from flair_amd.zone_detect import detect_convert, tile_grid
    S, H, W = 64, 150, 190
    K = S - 2 * m
    stride = K + dstride
    rng = np.random.default_rng(1000 * C + 10 * m + dstride + 8)
    grid = tile_grid((W, H), S, m, stride)
    n = len(grid)
    truth = _truth(rng, H, W, C)
    tiles = torch.from_numpy(grid).to(dev)
    tr = torch.from_numpy(truth).to(dev)
    # (a): class bytes up to C + 2, so predictions outside range(C) are dropped too
    preds = rng.integers(0, C + 2, size=(n, S, S)).astype(np.uint8)
    cm = torch.zeros(n, C, C, dtype=torch.int64, device=dev)
    pd = torch.from_numpy(preds).to(dev)
    _launch("flair_zone_window_confmat_preds", L.ptr(pd), n, C, S, m, L.ptr(tiles), L.ptr(tr), H, W, L.ptr(cm))
    assert np.array_equal(cm.cpu().numpy(), _window_cms(truth, preds[:, m:S - m, m:S - m], grid, S, m, C))
    # (b)
    lg = torch.from_numpy(rng.normal(0, 3, size=(n, C, S, S)).astype(np.float32)).to(dev)
    cls = detect_convert(lg, m, "argmax")[:, 0].cpu().numpy()
    cm.zero_()
    _launch("flair_zone_window_confmat_logits", L.ptr(lg), n, C, S, m, L.ptr(tiles), L.ptr(tr), H, W, L.ptr(cm))
    assert np.array_equal(cm.cpu().numpy(), _window_cms(truth, cls, grid, S, m, C))
    # (c)
    rast = np.zeros((2, H, W), np.float32)
    rast[0] = rng.integers(0, C, size=(H, W))
    rast[1] = rng.random((H, W))
    rd = torch.from_numpy(rast).to(dev)
    cm.zero_()
    _launch("flair_zone_window_confmat_raster", L.ptr(rd), n, C, S, m, L.ptr(tiles), L.ptr(tr), H, W, L.ptr(cm))
    K_cls = np.stack([rast[0, y0 + m:y0 + m + K, x0 + m:x0 + m + K] for x0, y0 in grid[:, :2]])
    assert np.array_equal(cm.cpu().numpy(), _window_cms(truth, K_cls, grid, S, m, C))
    # the whole-raster count of the same band
    from flair_amd import zone_metrics as ZM
    assert np.array_equal(ZM.raster_confmat(rd, tr, C).cpu().numpy(), _confmat_np(truth, rast[0], C))


def _zcfg(C, **kw):
    c = {"img_pixels_detection": 64, "margin": 8, "output_type": "argmax", "n_classes": C, "batch_size": 4,
         "channels": [1, 2, 3, 4, 5], "norma_task": [{"norm_type": "custom", "norm_means": MEANS, "norm_stds": STDS}],
         "classes": _classes(C), "model_name": "test-model"}
    c.update(kw)
    return c


def _unet(dev, C, seed=2022):
    import flair_amd
    from oracle import unet_resnet34 as om
    hip = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=C, compute_dtype="f32")
    hip.load_state_dict(om.seeded_model(5, C, seed=seed).state_dict())
    return hip.to(dev).eval()


def _segformer_b1(dev, C):
    import flair_amd
    torch.manual_seed(7)
    return flair_amd.SegformerForSemanticSegmentation(num_channels=5, num_labels=C, depths=(2, 2, 2, 2), hidden_sizes=(64, 128, 320, 512),
                                                      decoder_hidden_size=256, compute_dtype="f32").to(dev).eval()


def test_exact_clipping_windows_sum_to_raster(dev):
    """(ii) stride = K and extents that are multiples of K: every pixel belongs to one window, so the windows' matrices
    (from the U-Net's class tiles) sum to the finished raster's matrix bit for bit, and each equals the raster's over its core"""
    from flair_amd import zone_metrics as ZM
    from flair_amd.zone_detect import ZoneDetector, tile_grid
    C, S, m = 13, 64, 8
    K = S - 2 * m
    H, W = 3 * K, 4 * K
    rng = np.random.default_rng(11)
    raster = torch.from_numpy(rng.integers(0, 256, size=(5, H, W), dtype=np.uint8)).to(dev)
    truth = _truth(rng, H, W, C)
    tr = torch.from_numpy(truth).to(dev)
    det = ZoneDetector(_unet(dev, C), _zcfg(C, stitching="exact-clipping", stride=K, padding="no-padding"))
    out = det.run(raster, tr)
    grid = tile_grid((W, H), S, m, K)
    assert len(grid) == (H // K) * (W // K) and det.window_confmats.shape == (len(grid), C, C)
    win = det.window_confmats.cpu().numpy()
    total = ZM.raster_confmat(out, tr, C).cpu().numpy()
    assert np.array_equal(win.sum(0), total)
    cls = out[0].cpu().numpy()
    assert np.array_equal(win, _window_cms(truth, np.stack([cls[y0 + m:y0 + m + K, x0 + m:x0 + m + K] for x0, y0 in grid[:, :2]]),
                                           grid, S, m, C))
    assert np.array_equal(det.window_rects, np.stack([grid[:, 0] + m, grid[:, 1] + m, np.full(len(grid), K), np.full(len(grid), K)], 1))
    # and without the truth the run is what it was
    again = det.run(raster)
    assert torch.equal(again, out) and det.window_confmats is None


def _error_map_np(truth, cls, S, m, stride):
    from scipy.ndimage import gaussian_filter
    from flair_amd.zone_detect import slice_pixels
    K = S - 2 * m
    target = truth - 1
    acc = np.zeros((K, K))
    patches = slice_pixels(truth.shape, S, m, stride)
    for x0, x1, y0, y1 in patches:
        acc += np.where(target[x0:x1, y0:y1] != cls[x0:x1, y0:y1], 1, 0)
    return gaussian_filter(acc / len(patches), sigma=2)


@pytest.mark.parametrize("S,m,stride", [(64, 8, 16), (64, 8, 48), (64, 0, 70), (20, 4, 5)])
def test_error_map_vs_scipy(dev, S, m, stride):
    """(iii) K = 12 < 17 taps exercises scipy's repeated reflection"""
    from flair_amd import zone_metrics as ZM
    H, W, C = 150, 190, 19
    rng = np.random.default_rng(S + m + stride)
    truth = _truth(rng, H, W, C)
    rast = np.zeros((2, H, W), np.float32)
    rast[0] = np.where(rng.random((H, W)) < 0.5, (truth.astype(np.int64) - 1) % C, rng.integers(0, C, size=(H, W)))
    got = ZM.error_map(torch.from_numpy(rast).to(dev), torch.from_numpy(truth).to(dev), S, m, stride).cpu().numpy()
    want = _error_map_np(truth, rast[0], S, m, stride)
    assert got.dtype == np.float64 and got.shape == want.shape
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_error_map_and_records_vs_reference_fixture(dev, golden_dir):
    """(iii) the reference's own error_rate_patch map, and its compute_metrics_patch records from device-counted matrices"""
    from flair_amd import _lib as L
    from flair_amd import zone_metrics as ZM
    with open(os.path.join(golden_dir, "zone_metrics_reference.json")) as f:
        meta = json.load(f)
    arr = np.load(os.path.join(golden_dir, "zone_metrics_reference.npz"))
    H, W = meta["raster_hw"]
    S, m, st = meta["patch_size"], meta["margin"], meta["stride"]
    K, C = S - 2 * m, len(meta["classes"])
    rast = np.zeros((2, H, W), np.float32)
    rast[0] = arr["pred"]
    rd, tr = torch.from_numpy(rast).to(dev), torch.from_numpy(arr["truth"]).to(dev)
    got = ZM.error_map(rd, tr, S, m, st).cpu().numpy()
    np.testing.assert_allclose(got, arr["error_map"], rtol=0, atol=1e-12)
    cfg = {"classes": {int(k): v for k, v in meta["classes"].items()}}
    rects = np.asarray([[int(v) for v in next(iter(r)).rsplit("_", 2)[1:]] + [K, K] for r in meta["window_records"]], np.int32)
    tiles = torch.from_numpy(np.concatenate([rects[:, :2] - m, np.zeros((len(rects), 4), np.int64)], 1).astype(np.int32)).to(dev)
    cm = torch.zeros(len(rects), C, C, dtype=torch.int64, device=dev)
    _launch("flair_zone_window_confmat_raster", L.ptr(rd), len(rects), C, S, m, L.ptr(tiles), L.ptr(tr), H, W, L.ptr(cm))
    recs = ZM.window_records(meta["method"], cm.cpu().numpy(), rects, cfg)
    for g, w in zip(recs, meta["window_records"]):
        assert list(g) == list(w)
        gv, wv = next(iter(g.values())), next(iter(w.values()))
        assert list(gv) == list(wv)
        for k in ("Avg_metrics", "per_class_iou", "per_class_fscore"):
            np.testing.assert_allclose(gv[k], wv[k], rtol=1e-9, atol=1e-9)


def _own_window_classes(det, model, raster, grid):
    """each window's own class map (K, K), computed apart from run(): gather, model, crop"""
    from flair_amd import _lib as L
    from flair_amd.data_feed import NORM_CODES
    from flair_amd.zone_detect import detect_convert
    dev = raster.device
    _, H, W = raster.shape
    S, m = det.S, det.margin
    out = []
    for b0 in range(0, len(grid), det.batch_size):   # the run's own batches
        t = torch.from_numpy(grid[b0:b0 + det.batch_size]).to(dev).contiguous()
        B = t.shape[0]
        imgs = torch.empty(B, 5, S, S, dtype=torch.float32, device=dev)
        L.check(L.lib().flair_gather_tiles(L.ptr(raster), 5, H, W, L.ptr(t), B, S, det._ch, 5, NORM_CODES[det.norm_type], det._means,
                                           det._stds, L.ptr(imgs), L.stream()))
        with torch.no_grad():
            if det._fast_preds(0):
                out.append(model.predict_classes(imgs, want_prob=True)[0][:, m:S - m, m:S - m].cpu().numpy())
            else:
                out.append(detect_convert(det._logits(imgs), m, "argmax")[:, 0].cpu().numpy())
    return np.concatenate(out)


@pytest.mark.parametrize("which", ["unet", "segformer_b1"])
def test_evaluate_end_to_end(dev, which):
    """(iv) every stitching method: records equal a host computation from the returned rasters (overlap methods)
    or from the windows' own class maps (exact clipping); rasters equal compare(); nothing changes when the batch is split"""
    from flair_amd import zone_metrics as ZM
    from flair_amd.zone_detect import ZoneDetector, compare, tile_grid
    C = 13 if which == "unet" else 19
    model = _unet(dev, C) if which == "unet" else _segformer_b1(dev, C)
    # SegFormer tiles: (S/32)^2 a multiple of 16
    S, m, H, W = (64, 8, 150, 190) if which == "unet" else (128, 32, 200, 264)
    stride = S // 4
    rng = np.random.default_rng(31)
    raster = torch.from_numpy(rng.integers(0, 256, size=(5, H, W), dtype=np.uint8)).to(dev)
    truth = _truth(rng, H, W, C)
    tr = torch.from_numpy(truth).to(dev)
    strat = {"tiling": {"enabled": True, "size_range": [S], "stride_range": [0.25]},
             "stitching": {"enabled": True, "methods": list(METHODS), "margin": [m]}}
    cfg = _zcfg(C, img_pixels_detection=S, margin=m, overlap_strat=True, strategies=strat, model_name=which)
    res = ZM.evaluate(model, cfg, raster, tr)
    ref = compare(model, cfg, raster)
    assert list(res) == list(ref) and len(res) == 4
    split = ZM.evaluate(model, dict(cfg, batch_size=3), raster, tr)
    K = S - 2 * m
    grid = tile_grid((W, H), S, m, stride)
    own = None
    for name, r in res.items():
        meth = ZM.parse_method(name)["stitching"]
        assert torch.equal(r["raster"], ref[name][0]), name
        assert r["ms"] > 0 and r["metrics_ms"] > 0
        if meth == "exact-clipping":
            if own is None:
                det = ZoneDetector(model, dict(cfg, stitching=meth, stride=stride, padding="no-padding"))
                own = _own_window_classes(det, model, raster, grid)
            cls = own
        else:
            band = r["raster"][0].cpu().numpy()
            cls = np.stack([band[y0 + m:y0 + m + K, x0 + m:x0 + m + K] for x0, y0 in grid[:, :2]])
        cms = _window_cms(truth, cls, grid, S, m, C)
        rects = np.stack([grid[:, 0] + m, grid[:, 1] + m, np.full(len(grid), K), np.full(len(grid), K)], 1)
        assert r["window_records"] == ZM.window_records(name, cms, rects, cfg), name
        total = _confmat_np(truth, r["raster"][0].cpu().numpy(), C)
        assert np.array_equal(r["confmat"], total) and r["confmat"].dtype == np.int64
        assert r["record"] == ZM.method_record(name, total, cfg, r["ms"])
        assert r["record"]["Parameters values"] == [which, S, stride, m, "no-padding", meth]
        np.testing.assert_allclose(r["error_map"], _error_map_np(truth, r["raster"][0].cpu().numpy(), S, m, stride), rtol=0, atol=1e-12)
        s = split[name]
        assert torch.equal(s["raster"], r["raster"]) and s["window_records"] == r["window_records"], name
        assert np.array_equal(s["confmat"], r["confmat"]) and np.array_equal(s["error_map"], r["error_map"]), name


def test_aggregate_two_zones(dev):
    """(v) batch_metrics over two zones: one summed matrix per method, records rebuilt from it, error maps averaged"""
    from flair_amd import zone_metrics as ZM
    C = 13
    model = _unet(dev, C)
    rng = np.random.default_rng(41)
    strat = {"tiling": {"enabled": True, "size_range": [64], "stride_range": [0.5]},
             "stitching": {"enabled": True, "methods": ["exact-clipping", "average_weights"], "margin": [8]}}
    cfg = _zcfg(C, overlap_strat=True, strategies=strat)
    zones = []
    for H, W in ((96, 128), (120, 100)):
        raster = torch.from_numpy(rng.integers(0, 256, size=(5, H, W), dtype=np.uint8)).to(dev)
        zones.append(ZM.evaluate(model, cfg, raster, torch.from_numpy(_truth(rng, H, W, C)).to(dev)))
    agg = ZM.aggregate(zones, cfg)
    assert list(agg) == list(zones[0])
    for name, a in agg.items():
        total = zones[0][name]["confmat"] + zones[1][name]["confmat"]
        assert np.array_equal(a["confmat"], total)
        assert a["record"] == ZM.method_record(name, total, cfg, (zones[0][name]["ms"] + zones[1][name]["ms"]) / 2)
        np.testing.assert_allclose(a["error_map"], (zones[0][name]["error_map"] + zones[1][name]["error_map"]) / 2, rtol=0, atol=1e-15)


def test_truth_is_checked(dev):
    from flair_amd.zone_detect import ZoneDetector
    C = 13
    model = _unet(dev, C)
    raster = torch.zeros(5, 96, 96, dtype=torch.uint8, device=dev)
    det = ZoneDetector(model, _zcfg(C))
    with pytest.raises(ValueError, match="extent"):
        det.run(raster, torch.zeros(96, 95, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="class_prob"):
        ZoneDetector(model, _zcfg(C, output_type="class_prob")).run(raster, torch.zeros(96, 96, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="classes"):
        ZoneDetector(model, _zcfg(C, classes=_classes(19))).run(raster, torch.zeros(96, 96, dtype=torch.uint8, device=dev))


def test_abi_rejects_bad_arguments(dev):
    from flair_amd import _lib as L
    lib = L.lib()
    t = torch.zeros(1, 6, dtype=torch.int32, device=dev)
    tr = torch.zeros(64, 64, dtype=torch.uint8, device=dev)
    r = torch.zeros(2, 64, 64, device=dev)
    cm = torch.zeros(33, 33, dtype=torch.int64, device=dev)
    assert lib.flair_zone_window_confmat_raster(L.ptr(r), 1, 33, 32, 0, L.ptr(t), L.ptr(tr), 64, 64, L.ptr(cm), L.stream()) == -2
    assert lib.flair_zone_window_confmat_preds(None, 1, 13, 32, 0, L.ptr(t), L.ptr(tr), 64, 64, L.ptr(cm), L.stream()) == -1
    assert lib.flair_zone_raster_confmat(L.ptr(r), L.ptr(tr), 64, 64, 0, L.ptr(cm), L.stream()) == -2
    ys = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.zeros(64 * 64 * 8, dtype=torch.uint8, device=dev)
    assert lib.flair_zone_error_map(L.ptr(r), L.ptr(tr), 64, 64, 65, L.ptr(ys), 1, L.ptr(ys), 1, 2.0, 8, L.ptr(ws), L.ptr(ws), L.ptr(ws),
                                    L.ptr(ws), L.ptr(ws), L.stream()) == -2
    torch.cuda.synchronize()
