#!/usr/bin/env python3
"""Generate tests/golden/zone_metrics_reference.{npz,json} by running the REFERENCE's own zone_detect metrics.

Run in the build container only (needs the reference checkout, read-only; GPU tests read only the committed data):

    python tests/golden/make_golden_zone_metrics.py [REFERENCE_ROOT]

What is executed from the reference (unchanged, imported as its package src.zone_detect.test.metrics):
  * compute_metrics_patch   per-window records (metrics.py:124-192), a few windows, edge windows included
  * clean_confmat + class_IoU / overall_accuracy / class_fscore / class_precision / class_recall on a summed matrix
  * error_rate_patch(save=False)   the smoothed error-rate map (metrics.py:350-442)
  * extract_method          on an 'average_weights' method name (utils.py:170-188): the IndexError it raises

``rasterio`` is absent here; it is replaced in ``sys.modules`` by an in-memory stand-in (``open`` of a registered array,
``windows.Window`` as a record of offsets) that carries no arithmetic of the path.  19 classes with the weight-0 classes of
configs/config_detect_compare_metrics.yaml (15, 16, 17, 19) and truth zeros, so the uint8 wrap 0 -> 255 is exercised.

Outputs are DATA only (inputs + expected outputs); no reference source text is stored.
"""
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"

ARRAYS = {}   # path -> array, what the stand-in rasterio.open(path).read(1) returns


def _install_rasterio():
    rio = types.ModuleType("rasterio")
    win = types.ModuleType("rasterio.windows")

    class Window:
        def __init__(self, col_off, row_off, width, height):
            self.col_off, self.row_off, self.width, self.height = col_off, row_off, width, height

    class _Src:
        def __init__(self, path):
            self.path = str(path)

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def read(self, band):
            a = ARRAYS[self.path]
            return a[band - 1] if a.ndim == 3 else a

    rio.open = lambda path, *a, **k: _Src(path)
    win.Window = Window
    rio.windows = win
    sys.modules.update({"rasterio": rio, "rasterio.windows": win})
    return Window


WEIGHTS = {c: 1 for c in range(1, 20)}
WEIGHTS.update({15: 0, 16: 0, 17: 0, 19: 0})
NAMES = ["building", "pervious surface", "impervious surface", "bare soil", "water", "coniferous", "deciduous", "brushwood",
         "vineyard", "herbaceous vegetation", "agricultural land", "plowed land", "swimming_pool", "snow", "clear cut", "mixed",
         "ligneous", "greenhouse", "other"]
C = 19
H, W, S, M, STRIDE = 70, 90, 32, 4, 12
K = S - 2 * M


def _rasters(seed):
    rng = np.random.default_rng(seed)
    truth = rng.integers(0, C + 1, size=(H, W)).astype(np.uint8)      # 0 = no data
    truth[:K // 2, :K] = 0                                            # half of the first window is no data
    agree = rng.random((H, W)) < 0.6
    pred = np.where(agree, (truth.astype(np.int64) - 1) % 256, rng.integers(0, C, size=(H, W)))
    pred = np.where(pred >= C, rng.integers(0, C, size=(H, W)), pred).astype(np.uint8)
    return truth, pred


def main():
    Window = _install_rasterio()
    sys.path.insert(0, REF)
    from src.zone_detect.test import metrics as RM   # noqa: E402
    from src.zone_detect import utils as RU   # noqa: E402
    from sklearn.metrics import confusion_matrix

    classes = {c: [WEIGHTS[c], NAMES[c - 1]] for c in range(1, C + 1)}
    tmp = tempfile.mkdtemp()
    zone_dir = os.path.join(tmp, "D037_2021", "UU_S1_4")
    truth_path = os.path.join(zone_dir, "truth.tif")
    config = {"classes": classes, "truth_path": truth_path, "input_img_path": os.path.join(zone_dir, "img.tif")}

    truth, pred = _rasters(2025)
    truth2, pred2 = _rasters(2026)
    pred_f32 = np.stack([pred.astype(np.float32), np.zeros((H, W), np.float32)])   # the (2, H, W) 'argmax' raster
    target = truth - 1   # uint8 arithmetic, utils.py:288

    method = f"size={S}_stride={STRIDE}_margin={M}_padding=no-padding_stitching=exact-clipping"
    windows = [(0, 0), (W - K, H - K), (W - K, 0), (0, H - K), (37, 11), (12, 40)]   # (col_off, row_off)
    records = []
    for c0, r0 in windows:
        rec = RM.compute_metrics_patch(pred_f32[:, r0:r0 + K, c0:c0 + K], target, Window(c0, r0, K, K), config, method)
        records.append({k: {kk: ([float(x) for x in vv] if kk in ("Avg_metrics", "per_class_iou", "per_class_fscore") else vv)
                            for kk, vv in v.items()} for k, v in rec.items()})

    summed = (confusion_matrix((truth - 1).flatten(), pred.flatten(), labels=range(C)).astype(np.float64)
              + confusion_matrix((truth2 - 1).flatten(), pred2.flatten(), labels=range(C)))
    cleaned = RM.clean_confmat(summed, config)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou, miou = RM.class_IoU(cleaned)
        oa = RM.overall_accuracy(cleaned)
        fs, mfs = RM.class_fscore(cleaned)
        pr, mpr = RM.class_precision(cleaned)
        rc, mrc = RM.class_recall(cleaned)

    pred_path = os.path.join(zone_dir, f"037_2021_UU_S1_4_IRC-ARGMAX-S_{method}.tif")
    ARRAYS[truth_path] = truth
    ARRAYS[pred_path] = pred_f32
    dic = RM.error_rate_patch(truth_file=truth_path, out_dir=os.path.join(tmp, "out"), pred_path=pred_path, dic={}, save=False)
    emap = dic[pred_path]

    try:
        RU.extract_method(f"size={S}_stride={STRIDE}_margin={M}_padding=no-padding_stitching=average_weights", {})
        aw_error = None
    except Exception as e:  # noqa: BLE001
        aw_error = type(e).__name__

    try:   # a window whose truth is no data only: sklearn refuses it
        RM.compute_metrics_patch(pred_f32[:, :K, :K], np.full((H, W), 255, np.uint8), Window(0, 0, K, K), config, method)
        nodata_error = None
    except Exception as e:  # noqa: BLE001
        nodata_error = type(e).__name__

    np.savez_compressed(os.path.join(HERE, "zone_metrics_reference.npz"), truth=truth, pred=pred, truth2=truth2, pred2=pred2,
                        summed_confmat=summed, error_map=emap)
    out = {
        "classes": {str(k): v for k, v in classes.items()},
        "raster_hw": [H, W], "patch_size": S, "margin": M, "stride": STRIDE, "method": method,
        "window_records": records,
        "summed": {"per_class_iou": iou.tolist(), "miou": float(miou), "overall_accuracy": float(oa),
                   "per_class_fscore": fs.tolist(), "mean_fscore": float(mfs), "per_class_precision": pr.tolist(),
                   "mean_precision": float(mpr), "per_class_recall": rc.tolist(), "mean_recall": float(mrc)},
        "error_map_patches": len(RM.slice_pixels((H, W), S, M, STRIDE)),
        "average_weights_extract_method_raises": aw_error,
        "no_data_window_compute_metrics_patch_raises": nodata_error,
    }
    with open(os.path.join(HERE, "zone_metrics_reference.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("wrote zone_metrics_reference.{npz,json}:", len(records), "window records,", out["error_map_patches"], "patches,",
          "average_weights ->", aw_error)


if __name__ == "__main__":
    main()
