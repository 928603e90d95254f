"""zone_detect metrics on the host (flair_amd.zone_metrics) against tests/golden/zone_metrics_reference.*, which the
reference's own compute_metrics_patch / clean_confmat / scores / error_rate_patch produced (make_golden_zone_metrics.py)."""
import json
import os

import numpy as np
import pytest

from flair_amd import zone_metrics as ZM
from flair_amd.zone_detect import STITCHING, gen_param_combination, method_name


@pytest.fixture(scope="module")
def gold(golden_dir):
    with open(os.path.join(golden_dir, "zone_metrics_reference.json")) as f:
        meta = json.load(f)
    arr = dict(np.load(os.path.join(golden_dir, "zone_metrics_reference.npz")))
    meta["config"] = {"classes": {int(k): v for k, v in meta["classes"].items()}, "model_name": "unet"}
    return meta, arr


def _confmat_np(truth_u8, pred, C):
    """sklearn.confusion_matrix(truth - 1, pred, labels=range(C)) in numpy: pairs outside range(C) dropped"""
    t = (truth_u8.astype(np.int64) - 1) % 256
    p = np.asarray(pred).astype(np.int64)
    ok = (t < C) & (p >= 0) & (p < C)
    return np.bincount(t[ok] * C + p[ok], minlength=C * C).reshape(C, C)


def _close(a, b, tol=1e-9):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    np.testing.assert_allclose(a, b, rtol=tol, atol=tol, equal_nan=True)


def test_window_records_match_reference(gold):
    meta, arr = gold
    cfg, C = meta["config"], len(meta["classes"])
    K = meta["patch_size"] - 2 * meta["margin"]
    rects, cms = [], []
    for rec in meta["window_records"]:
        key = next(iter(rec))
        c0, r0 = (int(v) for v in key.rsplit("_", 2)[1:])
        rects.append((c0, r0, K, K))
        cms.append(_confmat_np(arr["truth"][r0:r0 + K, c0:c0 + K], arr["pred"][r0:r0 + K, c0:c0 + K], C))
    got = ZM.window_records(meta["method"], np.stack(cms), np.asarray(rects), cfg)
    assert len(got) == len(meta["window_records"])
    for g, w in zip(got, meta["window_records"]):
        assert list(g) == list(w)                       # the key: method_col_row
        gv, wv = next(iter(g.values())), next(iter(w.values()))
        assert list(gv) == list(wv)                     # the same fields in the same order
        assert gv["Avg_metrics_name"] == wv["Avg_metrics_name"] and gv["classes"] == wv["classes"]
        assert len(gv["classes"]) == C and len(gv["per_class_iou"]) == C - 4   # names uncleaned, scores cleaned
        for f in ("Avg_metrics", "per_class_iou", "per_class_fscore"):
            _close(gv[f], wv[f])


def test_summed_scores_match_reference(gold):
    meta, arr = gold
    cfg, want = meta["config"], meta["summed"]
    summed = arr["summed_confmat"]
    # the matrix itself is sklearn's over two rasters, summed as batch_metrics sums zones
    C = len(meta["classes"])
    assert np.array_equal(summed, _confmat_np(arr["truth"], arr["pred"], C) + _confmat_np(arr["truth2"], arr["pred2"], C))
    cm = ZM.clean_confmat(summed, cfg)
    assert cm.shape == (C - 4, C - 4)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou, miou = ZM.class_IoU(cm)
        fs, mfs = ZM.class_fscore(cm)
        pr, mpr = ZM.class_precision(cm)
        rc, mrc = ZM.class_recall(cm)
        oa = ZM.overall_accuracy(cm)
    _close(iou, want["per_class_iou"]); _close(miou, want["miou"])
    _close(fs, want["per_class_fscore"]); _close(mfs, want["mean_fscore"])
    _close(pr, want["per_class_precision"]); _close(mpr, want["mean_precision"])
    _close(rc, want["per_class_recall"]); _close(mrc, want["mean_recall"])
    _close(oa, want["overall_accuracy"])
    # the int64 matrix the device returns gives the same record as the reference's float64 sum
    rec = ZM.method_record(meta["method"], summed.astype(np.int64), cfg, 12.5)
    _close(rec["Avg_metrics"], [want["miou"], want["overall_accuracy"], want["mean_fscore"], 12.5])
    assert rec["Parameters values"] == ["unet", meta["patch_size"], meta["stride"], meta["margin"], "no-padding", "exact-clipping"]
    assert rec["Avg_metrics_name"] == ["mIoU", "Overall Accuracy", "Fscore", "Time in ms"]


def _error_map_np(truth, pred, S, m, stride):
    """error_rate_patch restated: mean over slice_pixels patches of (truth - 1 != pred), then scipy's gaussian_filter"""
    from scipy.ndimage import gaussian_filter
    from flair_amd.zone_detect import slice_pixels
    K = S - 2 * m
    target = truth - 1
    acc = np.zeros((K, K))
    patches = slice_pixels(truth.shape, S, m, stride)
    for x0, x1, y0, y1 in patches:
        acc += np.where(target[x0:x1, y0:y1] != pred[x0:x1, y0:y1].astype(np.float32), 1, 0)
    return gaussian_filter(acc / len(patches), sigma=2)


def test_error_map_restatement_matches_reference(gold):
    """the restatement the GPU test compares the device map against reproduces the reference's map; the comb-sum origins
    of error_origins make the same patch set"""
    meta, arr = gold
    S, m, st = meta["patch_size"], meta["margin"], meta["stride"]
    np.testing.assert_allclose(_error_map_np(arr["truth"], arr["pred"], S, m, st), arr["error_map"], rtol=0, atol=1e-15)
    rows, cols = ZM.error_origins(*meta["raster_hw"], S, m, st)
    assert len(rows) * len(cols) == meta["error_map_patches"]
    # the comb sums of the kernel, in numpy: R[r, j] = sum_x M[r, x + j], then E[i, j] = sum_y R[y + i, j]
    K = S - 2 * m
    M = ((arr["truth"] - 1) != arr["pred"].astype(np.float32)).astype(np.int64)
    R = sum(M[:, x:x + K] for x in cols)
    E = sum(R[y:y + K] for y in rows)
    from scipy.ndimage import gaussian_filter
    np.testing.assert_allclose(gaussian_filter(E / (len(rows) * len(cols)), sigma=2), arr["error_map"], rtol=0, atol=1e-12)


def test_parse_method_all_four_methods(gold):
    meta, _ = gold
    assert meta["average_weights_extract_method_raises"] == "IndexError"   # the reference's parser
    for stitch in STITCHING:
        combi = {"img_pixels_detection": 512, "stride": 128, "margin": 64, "padding": "no-padding", "stitching": stitch}
        assert ZM.parse_method(method_name(combi)) == {"patch_size": 512, "stride": 128, "margin": 64, "padding": "no-padding",
                                                      "stitching": stitch}
    with pytest.raises(ValueError):
        ZM.parse_method("size=512_stride=128")


def test_parse_method_over_the_config_grid():
    cfg = {"img_pixels_detection": 512, "margin": 0, "overlap_strat": True,
           "strategies": {"tiling": {"enabled": True, "size_range": [128, 256], "stride_range": [0.75, 0.5]},
                          "stitching": {"enabled": True, "methods": list(STITCHING), "margin": [0.125]}}}
    for combi in gen_param_combination(cfg):
        info = ZM.parse_method(method_name(combi))
        assert (info["patch_size"], info["stride"], info["margin"], info["padding"], info["stitching"]) == (
            combi["img_pixels_detection"], combi["stride"], combi["margin"], combi["padding"], combi["stitching"])


def test_batched_scores_equal_per_window(gold):
    meta, _ = gold
    cfg, C = meta["config"], len(meta["classes"])
    rng = np.random.default_rng(3)
    cms = rng.integers(0, 50, size=(40, C, C)) * (rng.random((40, C, C)) < 0.3)
    cms[0] = 0                                   # an empty matrix: OA NaN, IoU / F-score 0
    cms[1, :, 3] = 0; cms[1, 3, :] = 0           # an absent class
    per_iou, miou, oa, per_f, mf = ZM.scores(cms, cfg)
    for n in range(len(cms)):
        one = ZM.clean_confmat(cms[n], cfg)
        with np.errstate(divide="ignore", invalid="ignore"):
            i1, mi1 = ZM.class_IoU(one)
            f1, mf1 = ZM.class_fscore(one)
            o1 = ZM.overall_accuracy(one)
        _close(per_iou[n], i1, 1e-12); _close(miou[n], mi1, 1e-12)
        _close(per_f[n], f1, 1e-12); _close(mf[n], mf1, 1e-12)
        _close(oa[n], o1, 1e-12)
    assert np.isnan(oa[0]) and miou[0] == 0 and mf[0] == 0
    rects = np.stack([np.arange(40), 2 * np.arange(40), np.full(40, 8), np.full(40, 8)], axis=1)
    recs = ZM.window_records("size=16_stride=8_margin=4_padding=no-padding_stitching=max", cms, rects, cfg)
    assert [next(iter(r)) for r in recs] == [f"size=16_stride=8_margin=4_padding=no-padding_stitching=max_{n}_{2 * n}" for n in range(40)]


def test_aggregate_sums_zones(gold):
    meta, _ = gold
    cfg, C = meta["config"], len(meta["classes"])
    rng = np.random.default_rng(5)
    meth = ["size=32_stride=12_margin=4_padding=no-padding_stitching=" + s for s in ("exact-clipping", "average_weights")]
    zones = [{mth: {"confmat": rng.integers(0, 100, size=(C, C)), "error_map": rng.random((24, 24)), "ms": float(10 + z)}
              for mth in meth} for z in range(3)]
    agg = ZM.aggregate(zones, cfg)
    assert list(agg) == meth
    for mth in meth:
        total = sum(z[mth]["confmat"] for z in zones)
        assert np.array_equal(agg[mth]["confmat"], total)
        np.testing.assert_allclose(agg[mth]["error_map"], sum(z[mth]["error_map"] for z in zones) / 3, rtol=0, atol=1e-15)
        want = ZM.method_record(mth, total, cfg, 11.0)
        assert agg[mth]["record"] == want and agg[mth]["zones"] == 3
    assert ZM.aggregate({"a": zones[0], "b": zones[1]}, cfg)[meth[0]]["zones"] == 2
