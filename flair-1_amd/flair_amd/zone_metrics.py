"""zone_detect's comparison metrics against a ground-truth raster (src/zone_detect/test/metrics.py, main.py:255-372 with
``--compare --metrics``).

The counting runs on the device (csrc/zone_metrics.hip): ``ZoneDetector.run(raster, truth)`` leaves one C x C confusion matrix
per window, ``raster_confmat`` counts a finished raster, ``error_map`` builds error_rate_patch's K x K map.  Only those small
arrays come to the host, where the scores are plain numpy on (n, C, C) stacks: one copy for every window of a combination
instead of one sklearn call per window.

Semantics (metrics.py): the truth class is ``truth - 1`` in uint8 arithmetic, so a stored 0 becomes 255 and is dropped by the
confusion matrix (labels=range(C)) but counts as an error in the error map; classes of weight 0 leave the matrix before scoring;
scores are percentages with NaN set to 0 (overall accuracy excepted, as in the reference).  Deviations: DESIGN §8 D1-D4.
"""
from __future__ import annotations

import re
import time

import numpy as np
import torch

from . import _lib as L
from . import zone_detect as Z

AVG_METRICS_NAME = ["mIoU", "Overall Accuracy", "Fscore"]
METHOD_PARAMETERS = ["model name", "patch size", "stride", "margin", "padding", "stitching method"]
ERROR_SIGMA, ERROR_TRUNCATE = 2.0, 4.0   # scipy.ndimage.gaussian_filter(out_array, sigma=2) and its default truncate


# ------------------------------------------------------------------------------------------------------------------
# Scores (metrics.py:18-29, 88-120).  Every function takes one (C, C) matrix or a stack (..., C, C): rows truth, columns
# prediction; per-class results run along the last axis, averages over it.

def clean_confmat(confmat: np.ndarray, config: dict) -> np.ndarray:
    """metrics.py:18-29: drop the rows and columns of the classes whose weight in config['classes'] is 0."""
    weights = np.array([class_info[0] for class_info in config["classes"].values()])
    unused = np.where(weights == 0)[0]
    if unused.size > 0:
        return np.delete(np.delete(confmat, unused, axis=-2), unused, axis=-1)
    return confmat


def _diag(npcm):
    return np.diagonal(npcm, axis1=-2, axis2=-1)


def overall_accuracy(npcm):
    """100 * trace / sum (NaN when the matrix is empty, as in the reference)."""
    return 100 * (_diag(npcm).sum(axis=-1) / npcm.sum(axis=(-2, -1)))


def class_IoU(npcm):
    ious = 100 * _diag(npcm) / (np.sum(npcm, axis=-1) + np.sum(npcm, axis=-2) - _diag(npcm))
    ious[np.isnan(ious)] = 0
    return ious, np.mean(ious, axis=-1)


def class_precision(npcm):
    precision = 100 * _diag(npcm) / np.sum(npcm, axis=-2)
    precision[np.isnan(precision)] = 0
    return precision, np.mean(precision, axis=-1)


def class_recall(npcm):
    recall = 100 * _diag(npcm) / np.sum(npcm, axis=-1)
    recall[np.isnan(recall)] = 0
    return recall, np.mean(recall, axis=-1)


def class_fscore(npcm):
    """2PR / (P + R) from class_precision and class_recall (zone_detect's form: it takes the confusion matrix)."""
    precision = class_precision(npcm)[0]
    recall = class_recall(npcm)[0]
    fscore = 2 * (precision * recall) / (precision + recall)
    fscore[np.isnan(fscore)] = 0
    return fscore, np.mean(fscore, axis=-1)


def scores(confmats: np.ndarray, config: dict):
    """(per-class IoU, mIoU, OA, per-class F-score, mean F-score) of cleaned matrices, batched over leading axes."""
    cm = clean_confmat(np.asarray(confmats), config)
    with np.errstate(divide="ignore", invalid="ignore"):
        per_iou, miou = class_IoU(cm)
        oa = overall_accuracy(cm)
        per_f, mf = class_fscore(cm)
    return per_iou, miou, oa, per_f, mf


def _class_names(config: dict) -> list:
    classes = config["classes"]
    return [classes[i][1] for i in range(1, len(classes) + 1)]


# ------------------------------------------------------------------------------------------------------------------
# Records (metrics.py:124-287)

def parse_method(name: str) -> dict:
    """The parameters of a method name (main.py:302).  The reference's extract_method (utils.py:170-188) splits on '_' and
    raises IndexError on 'stitching=average_weights' (DESIGN §8 D3); the five keys are matched here instead."""
    m = re.fullmatch(r"size=(\d+)_stride=(\d+)_margin=(\d+)_padding=(.+?)_stitching=(.+)", name)
    if m is None:
        raise ValueError(f"not a zone_detect method name: {name!r}")
    return {"patch_size": int(m.group(1)), "stride": int(m.group(2)), "margin": int(m.group(3)), "padding": m.group(4),
            "stitching": m.group(5)}


def window_records(method: str, confmats: np.ndarray, rects: np.ndarray, config: dict) -> list:
    """compute_metrics_patch (metrics.py:124-192) for every window, in job order: [{f"{method}_{col_off}_{row_off}": record}]."""
    per_iou, miou, oa, per_f, mf = scores(confmats, config)
    names = _class_names(config)
    out = []
    for n in range(len(rects)):
        out.append({f"{method}_{int(rects[n, 0])}_{int(rects[n, 1])}": {
            "Avg_metrics_name": list(AVG_METRICS_NAME),
            "Avg_metrics": [float(miou[n]), float(oa[n]), float(mf[n])],
            "classes": list(names),
            "per_class_iou": per_iou[n].tolist(),
            "per_class_fscore": per_f[n].tolist()}})
    return out


def method_record(method: str, confmat: np.ndarray, config: dict, ms: float) -> dict:
    """batch_metrics (metrics.py:195-287) for one method from its summed confusion matrix; 'Time in ms' is ``ms``
    (DESIGN §8 D2)."""
    per_iou, miou, oa, per_f, mf = scores(confmat, config)
    info = parse_method(method)
    return {"Method parameters": list(METHOD_PARAMETERS),
            "Parameters values": [config.get("model_name"), info["patch_size"], info["stride"], info["margin"], info["padding"],
                                  info["stitching"]],
            "Avg_metrics_name": AVG_METRICS_NAME + ["Time in ms"],
            "Avg_metrics": [float(miou), float(oa), float(mf), float(ms)],
            "classes": _class_names(config),
            "per_class_iou": per_iou.tolist(),
            "per_class_fscore": per_f.tolist()}


# ------------------------------------------------------------------------------------------------------------------
# Device counting

def _check_pair(raster: torch.Tensor, truth_u8: torch.Tensor):
    if not raster.is_cuda or raster.dtype != torch.float32 or raster.dim() != 3 or raster.shape[0] != 2:
        raise ValueError("raster must be the (2, H, W) float32 'argmax' output on the HIP device")
    if not truth_u8.is_cuda or truth_u8.dtype != torch.uint8 or tuple(truth_u8.shape) != tuple(raster.shape[1:]):
        raise ValueError("truth must be an (H, W) uint8 tensor on the HIP device, the raster's extent")
    return raster.contiguous(), truth_u8.contiguous()


def raster_confmat(raster: torch.Tensor, truth_u8: torch.Tensor, n_classes: int) -> torch.Tensor:
    """confusion_matrix(truth - 1, band 0, labels=range(C)) over the whole raster (metrics.py:236-238), int64 (C, C) on the device."""
    raster, truth_u8 = _check_pair(raster, truth_u8)
    cm = torch.zeros(n_classes, n_classes, dtype=torch.int64, device=raster.device)
    L.check(L.lib().flair_zone_raster_confmat(L.ptr(raster), L.ptr(truth_u8), raster.shape[1], raster.shape[2], int(n_classes),
                                              L.ptr(cm), L.stream()), "flair_zone_raster_confmat")
    return cm


def error_origins(raster_h: int, raster_w: int, patch_size: int, margin: int, stride: int):
    """Row and column origins of error_rate_patch's patches: slice_pixels((H, W), S, m, stride) passes (rows, cols) as
    (x, y) and slices rows with the x range (metrics.py:393-407), so its boxes are the grid rows x cols."""
    boxes = Z.slice_pixels((raster_h, raster_w), patch_size, margin, stride)
    rows = sorted({b[0] for b in boxes})
    cols = sorted({b[2] for b in boxes})
    if len(rows) * len(cols) != len(boxes):
        raise AssertionError("slice_pixels boxes are not a grid")
    return np.asarray(rows, dtype=np.int32), np.asarray(cols, dtype=np.int32)


def error_map(raster: torch.Tensor, truth_u8: torch.Tensor, patch_size: int, margin: int, stride: int) -> torch.Tensor:
    """error_rate_patch (metrics.py:350-442) of band 0 against truth - 1: the mean over the slice_pixels patches of the K x K
    map [target != pred] (no-data counts as an error), smoothed by gaussian_filter(sigma=2, mode='reflect') — fp64 (K, K) on
    the device."""
    raster, truth_u8 = _check_pair(raster, truth_u8)
    H, W = raster.shape[1], raster.shape[2]
    K = int(patch_size) - 2 * int(margin)
    if K < 1 or K > H or K > W:
        raise ValueError("the margin-cropped patch does not fit the raster")
    rows, cols = error_origins(H, W, patch_size, margin, stride)
    if rows.min() < 0 or rows.max() + K > H or cols.min() < 0 or cols.max() + K > W:
        raise AssertionError("a slice_pixels patch leaves the raster")
    dev = raster.device
    ys, xs = torch.from_numpy(rows).to(dev), torch.from_numpy(cols).to(dev)
    mask = torch.empty(H, W, dtype=torch.uint8, device=dev)
    colsum = torch.empty(H, K, dtype=torch.int32, device=dev)
    counts = torch.empty(K, K, dtype=torch.int32, device=dev)
    tmp = torch.empty(K, K, dtype=torch.float64, device=dev)
    out = torch.empty(K, K, dtype=torch.float64, device=dev)
    radius = int(ERROR_TRUNCATE * ERROR_SIGMA + 0.5)
    L.check(L.lib().flair_zone_error_map(L.ptr(raster), L.ptr(truth_u8), H, W, K, L.ptr(ys), len(rows), L.ptr(xs), len(cols),
                                         ERROR_SIGMA, radius, L.ptr(mask), L.ptr(colsum), L.ptr(counts), L.ptr(tmp), L.ptr(out),
                                         L.stream()), "flair_zone_error_map")
    return out


# ------------------------------------------------------------------------------------------------------------------
# The comparison loop with metrics, and its aggregation over zones

def evaluate(model, config: dict, raster_u8: torch.Tensor, truth_u8: torch.Tensor) -> dict:
    """``flair-detect --compare --metrics`` on one zone: for every combination of gen_param_combination(config),
    {method name: {"raster", "ms", "window_records", "confmat", "record", "error_map", "metrics_ms"}}.

    raster / ms are what compare() returns (ms: the synchronised wall time of ZoneDetector.run, which with the truth also
    counts each window's matrix as it goes, main.py:350-366); window_records are compute_metrics_patch's records in job order;
    confmat is the int64 (C, C) matrix of the finished class band (batch_metrics before its sum over zones); record is
    batch_metrics' record of this zone alone; error_map is error_rate_patch's fp64 (K, K) map; metrics_ms is the synchronised
    wall time of everything after the run (whole-raster count, error map, copies, host scores)."""
    results = {}
    for combi in Z.gen_param_combination(config):
        cfg = dict(config)
        cfg.update(combi)
        method = Z.method_name(combi)
        det = Z.ZoneDetector(model, cfg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = det.run(raster_u8, truth_u8)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        t1 = time.perf_counter()
        cm_dev = raster_confmat(out, truth_u8, det.n_classes)
        emap_dev = error_map(out, truth_u8, det.S, det.margin, det.stride)
        win = det.window_confmats.cpu().numpy()
        cm = cm_dev.cpu().numpy()
        emap = emap_dev.cpu().numpy()
        records = window_records(method, win, det.window_rects, cfg)
        rec = method_record(method, cm, cfg, ms)
        metrics_ms = (time.perf_counter() - t1) * 1e3
        results[method] = {"raster": out, "ms": ms, "window_records": records, "confmat": cm, "record": rec, "error_map": emap,
                           "metrics_ms": metrics_ms}
    return results


def aggregate(results_by_zone, config: dict) -> dict:
    """batch_metrics (metrics.py:195-287) + error_rate_loop (:290-347) over zones: ``results_by_zone`` is an iterable of
    evaluate() results (or a {zone: result} dict).  Per method: the summed confusion matrix, its record ('Time in ms' = the mean
    of the zones' run times), the error maps averaged over zones, and the number of zones."""
    if isinstance(results_by_zone, dict):
        results_by_zone = list(results_by_zone.values())
    acc = {}
    for zone in results_by_zone:
        for method, r in zone.items():
            a = acc.get(method)
            if a is None:
                acc[method] = {"confmat": np.asarray(r["confmat"], dtype=np.int64).copy(), "error_map": np.array(r["error_map"], dtype=np.float64),
                               "ms": [r["ms"]], "zones": 1}
            else:
                a["confmat"] += r["confmat"]
                a["error_map"] += r["error_map"]
                a["ms"].append(r["ms"])
                a["zones"] += 1
    out = {}
    for method, a in acc.items():
        ms = float(np.mean(a["ms"]))
        out[method] = {"confmat": a["confmat"], "record": method_record(method, a["confmat"], config, ms),
                       "error_map": a["error_map"] / a["zones"], "zones": a["zones"]}
    return out
