#!/usr/bin/env python3
"""Cost of zone_detect's comparison metrics (flair_amd.zone_metrics) next to the run they score: a synthetic 10,240 x 10,240 x 5
uint8 raster and a random 0..19 truth raster, 512-pixel windows, margin 128, 19 classes, argmax output.

Per combination: the synchronised wall time of ZoneDetector.run without the truth (what compare() times), with the truth (the
per-window matrices counted in the run), and of the metrics after the run (whole-raster matrix, error map, device-to-host
copies, host scores and records); metric cost = (with truth - without) + after.  Also the bytes the metrics copy to the host.
Default: the U-Net bf16 in all four stitching methods at stride 128; MODEL=segformer: SegFormer-MiT-B2 bf16, exact clipping at
the default stride 256.  Prints one JSON line per combination."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "flair-1_amd"))
import flair_amd  # noqa: E402
from flair_amd import zone_metrics as ZM  # noqa: E402
from flair_amd.zone_detect import ZoneDetector, method_name  # noqa: E402


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def main():
    dev = torch.device("cuda:0")
    side = int(os.environ.get("RASTER", "10240"))
    C = 19
    torch.manual_seed(2022)
    which = os.environ.get("MODEL", "unet")
    if which == "segformer":
        model = flair_amd.SegformerForSemanticSegmentation(num_channels=5, num_labels=C, compute_dtype="bf16").to(dev).eval()
        combos = [("exact-clipping", 256)]
    else:
        model = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=C, compute_dtype="bf16").to(dev).eval()
        combos = [(s, 128) for s in ("exact-clipping", "average", "average_weights", "max")]
    batch = int(os.environ.get("BATCH", "16" if which == "segformer" else "32"))
    cfg = {"img_pixels_detection": 512, "margin": 128, "output_type": "argmax", "n_classes": C, "batch_size": batch,
           "channels": [1, 2, 3, 4, 5], "padding": "no-padding", "model_name": which,
           "classes": {c: [0 if c in (15, 16, 17, 19) else 1, str(c)] for c in range(1, C + 1)},
           "norma_task": [{"norm_type": "custom", "norm_means": [105.08, 110.87, 101.82, 106.38, 53.26],
                           "norm_stds": [52.17, 45.38, 44, 39.69, 79.3]}]}
    raster = torch.randint(0, 256, (5, side, side), dtype=torch.uint8, device=dev)
    truth = torch.randint(0, C + 1, (side, side), dtype=torch.uint8, device=dev)
    for stitch, stride in combos:
        c = dict(cfg, stitching=stitch, stride=stride)
        name = method_name({"img_pixels_detection": 512, "stride": stride, "margin": 128, "padding": "no-padding", "stitching": stitch})
        det = ZoneDetector(model, c)
        det.run(raster[:, :2048, :2048].contiguous(), truth[:2048, :2048].contiguous())  # warm-up
        _, plain_ms = _timed(lambda: det.run(raster))
        out, truth_ms = _timed(lambda: det.run(raster, truth))

        def after():
            cm, cm_ms = _timed(lambda: ZM.raster_confmat(out, truth, C))
            emap, emap_ms = _timed(lambda: ZM.error_map(out, truth, det.S, det.margin, det.stride))
            t0 = time.perf_counter()
            host = (det.window_confmats.cpu().numpy(), cm.cpu().numpy(), emap.cpu().numpy())
            recs = ZM.window_records(name, host[0], det.window_rects, c)
            ZM.method_record(name, host[1], c, truth_ms)
            return host, recs, {"raster_confmat_ms": round(cm_ms, 2), "error_map_ms": round(emap_ms, 2),
                                "copies_and_records_ms": round((time.perf_counter() - t0) * 1e3, 2)}

        (host, recs, parts), after_ms = _timed(after)
        d2h = sum(a.nbytes for a in host)
        cost = truth_ms - plain_ms + after_ms
        print(json.dumps({"workload": f"zone_metrics {side}x{side}x5 uint8, {which} bf16, 19 classes, 512/128, {stitch} stride {stride}, "
                                      f"batch {batch}",
                          "windows": len(recs), "run_ms": round(plain_ms, 1), "run_with_truth_ms": round(truth_ms, 1),
                          "metrics_after_run_ms": round(after_ms, 1), "metric_cost_ms": round(cost, 1),
                          "metric_cost_share": round(cost / plain_ms, 4), **parts, "d2h_bytes": d2h}), flush=True)


if __name__ == "__main__":
    main()
