"""Device-side zone_detect.

The reference runs the model, takes ``softmax`` over classes, copies the FULL probability tensor to the host
(19 MiB per 512x512 tile at 19 classes) and then, per tile on the CPU, crops the margin and calls ``convert``
(src/zone_detect/compare.py:20-39,71-76; src/zone_detect/dataset.py:11-34).  ``inference`` below keeps the argument
list of the reference function; with ``fused=True`` (default) it returns the cropped, converted tiles
(2 x float32 per kept pixel for 'argmax', C bytes for 'class_prob') so that only those cross PCIe.

``ZoneDetector`` runs a whole raster resident in HBM: the default pipeline (exact clipping, main.py:386-428) and, for a
config holding one combination of the comparison grid (``gen_param_combination``, main.py:275-372), the overlap stitching
modes 'average', 'average_weights' and 'max' (compare.py:84-136 as DESIGN §8 states their intent), blended on the device
by the gather-form kernels of csrc/zone_stitch.hip.  ``compare`` is the comparison loop without file I/O or metrics;
``run(raster, truth)`` also counts every window's confusion matrix on the device, and ``zone_metrics.evaluate`` is the
comparison loop with metrics (main.py:255-372 with --metrics).

The HuggingFace-provider models (SegFormer, UperNet) classify at 1/4 of the tile size and the library resizes x4 (bilinear,
align_corners=False) to the tile.  A model with ``forward_quarter`` hands its (B, C, S/4, S/4) logits straight to the ``_q4``
kernels, which interpolate per output pixel in registers: the tile-sized fp32 tensor is never written.
``FLAIR_ZD_QUARTER=1`` / ``=0`` (read when a ``ZoneDetector`` is built) selects that path / the x4 pass and the full-resolution
kernels; unset, ``QUARTER_DEFAULT`` decides.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib as L
from .tta import tta_codes, tta_predict

OUTPUT_TYPES = {"argmax": 0, "class_prob": 1}   # the values config["output_type"] may take (compare.py:69-82)
_MODE_PROBS = 2                                   # private: every fp32 softmax probability, no convert (compare.py:35)
# ZoneDetector's path for models with forward_quarter when FLAIR_ZD_QUARTER is unset.  DESIGN §10 sets the bar for True: windows/s
# of scripts/bench_zone_detect.py (MODEL=segformer) and scripts/bench_upernet.py within 2 % of the x4 path's on the same box.
QUARTER_DEFAULT = False
_MAX_GRID_Y = 65535                               # windows per launch of the per-window confusion matrices (grid.y)


def detect_convert(logits: torch.Tensor, margin: int, output_type: str, upsample: int = 1, _probs: bool = False) -> torch.Tensor:
    """softmax(dim=1) -> [:, m:S-m, m:S-m] -> convert(., output_type) for a batch of square tiles.
    'argmax' -> float32 (B, 2, K, K); 'class_prob' -> uint8 (B, C, K, K).
    ``upsample=4``: the logits are (B, C, S/4, S/4) and are resized x4 (bilinear, align_corners=False) per output pixel inside
    the kernel; ``margin`` and K are in full-resolution pixels."""
    if not _probs and output_type not in OUTPUT_TYPES:
        raise ValueError("The output type has not been interpreted.")
    if upsample not in (1, 4):
        raise ValueError(f"upsample must be 1 or 4, not {upsample!r}")
    if logits.dim() != 4 or logits.shape[2] != logits.shape[3]:
        raise ValueError("logits must be (B, C, S, S)")
    logits = logits.detach().float().contiguous()
    B, C = logits.shape[:2]
    S = logits.shape[2] * upsample
    K = S - 2 * int(margin)
    if K < 1:
        raise ValueError("margin leaves no pixel")
    if _probs:
        out = torch.empty(B, C, K, K, dtype=torch.float32, device=logits.device)
    elif output_type == "argmax":
        out = torch.empty(B, 2, K, K, dtype=torch.float32, device=logits.device)
    else:
        out = torch.empty(B, C, K, K, dtype=torch.uint8, device=logits.device)
    name = "flair_detect_convert_q4" if upsample == 4 else "flair_detect_convert"
    L.check(getattr(L.lib(), name)(L.ptr(logits), B, C, S, int(margin), _MODE_PROBS if _probs else OUTPUT_TYPES[output_type], L.ptr(out),
                                   L.stream()), name)
    return out


def inference(device, model, use_gpu: bool, config: dict, samples: dict, fused: bool = True):
    """compare.py:20-39.  Returns (predictions, indices) as numpy arrays like the reference; with ``fused`` the
    predictions are already margin-cropped and converted to ``config['output_type']``."""
    if not use_gpu or torch.device(device).type != "cuda":
        raise RuntimeError("flair_amd.zone_detect.inference runs on a HIP device only")
    imgs = samples["image"].to(device, non_blocking=True)
    with torch.no_grad():
        up = 1
        if config.get("model_framework", {}).get("model_provider") == "HuggingFace":
            # the library's `.logits` of a SegFormer are 1/4 of the tile: softmax, margin crop and convert work at tile geometry,
            # so quarter logits go through the kernels that resize x4 per pixel, never through the full-resolution ones
            if hasattr(model, "forward_quarter") and imgs.shape[2] % 4 == 0 and imgs.shape[3] % 4 == 0:
                logits, up = model.forward_quarter(imgs), 4
            else:
                logits = model(imgs).logits
                if tuple(logits.shape[2:]) != tuple(imgs.shape[2:]):
                    raise ValueError(f"the model's .logits are {tuple(logits.shape[2:])} for tiles of {tuple(imgs.shape[2:])}: margin crop "
                                     "and convert need tile-sized logits, or a model with forward_quarter (1/4-size logits)")
        else:
            logits = model(imgs)
        if fused:
            predictions = detect_convert(logits, config["margin"], config["output_type"], upsample=up)
        else:   # the reference's own return value: every probability, uncropped (same HIP kernel, no ATen op on the path)
            predictions = detect_convert(logits, 0, "", upsample=up, _probs=True)
    indices = samples["index"].cpu().numpy()
    return predictions.cpu().numpy(), indices


# ------------------------------------------------------------------------------------------------------------------
# Default pipeline (exact clipping, default-sized tiling) over one raster resident in HBM — main.py:386-428.

def get_stride(config: dict) -> list:
    """src/zone_detect/test/tiles.py:4-15."""
    img_size = config["img_pixels_detection"]
    if not config.get("overlap_strat"):
        return [int(img_size - 2 * config["margin"])]
    return [int(i * img_size) for i in config["strategies"]["tiling"]["stride_range"]]


def _axis_origins(extent: int, patch: int, margin: int, step: int) -> list:
    """Window origins along one axis as slice_extent lays them out (slicing_job.py:52-67): start one margin before the
    raster, advance by ``step``, pull a window that would end past extent + margin back to end exactly there;
    repeats are dropped (slicing_job.py:86-95)."""
    out = []
    for o in range(-margin, extent + margin, step):
        if o + patch > extent + margin:
            o = extent + margin - patch
        if o not in out:
            out.append(o)
    return out


def tile_grid(img_size, patch_size: int, margin: int, stride: int | None = None):
    """Pixel-space slicing job.  img_size = (width, height).  Returns an (n, 6) int32 array of
    {x0, y0, wx0, wx1, wy0, wy1} in the job's order (columns outer, rows inner, rows counted from the BOTTOM of the
    raster like the reference's geographic Y axis): window origin (top-left, image coordinates) and the output
    rectangle the window owns once every later window of the job has been written over it."""
    import numpy as np
    W, H = int(img_size[0]), int(img_size[1])
    K = patch_size - 2 * margin
    step = int(stride) if stride else K
    if K < 1 or W < K or H < K:
        raise ValueError("raster smaller than the margin-cropped patch")
    xs = _axis_origins(W, patch_size, margin, step)
    ys = _axis_origins(H, patch_size, margin, step)  # distance of the window's bottom edge from the raster's bottom edge

    def owned(origins, extent):
        lo = [o + margin for o in origins]
        hi = [min(o + patch_size - margin, extent) for o in origins]
        return [(lo[i], min(hi[i], lo[i + 1]) if i + 1 < len(origins) else hi[i]) for i in range(len(origins))]

    ox, oy = owned(xs, W), owned(ys, H)
    rows = []
    for i, x in enumerate(xs):
        for j, yb in enumerate(ys):
            rows.append((x, H - (yb + patch_size), ox[i][0], ox[i][1], H - oy[j][1], H - oy[j][0]))
    return np.asarray(rows, dtype=np.int32)


STITCHING = ("exact-clipping", "average", "average_weights", "max")   # the methods of compare.py:67-136


def gen_param_combination(config: dict) -> list:
    """src/zone_detect/utils.py:110-166: every (padding, tile size, margin, stride, stitching) combination of the comparison
    grid, quirks included: the stitching methods are read from ``strategies.stitching.methods`` (the shipped YAML writes
    ``method``, which is ignored), a margin below 1 is a fraction of the tile size, combinations with size <= 2 * margin are
    skipped and the strides come from ``get_stride`` (so from ``stride_range`` only when ``overlap_strat`` is set)."""
    combi = []
    padding_list = config.get("strategies", {}).get("padding_overall", [])
    if not padding_list:
        padding_list = ["no-padding"]
    tiling_cfg = config.get("strategies", {}).get("tiling", {})
    if tiling_cfg.get("enabled", False):
        tile_size_list = tiling_cfg.get("size_range", [config["img_pixels_detection"]])
    else:
        tile_size_list = [config["img_pixels_detection"]]
    stitching_cfg = config.get("strategies", {}).get("stitching", {})
    if stitching_cfg.get("enabled", False):
        margin_list = stitching_cfg.get("margin", [config["margin"]])
        stitching_methods = stitching_cfg.get("methods", ["exact-clipping"])
    else:
        margin_list = [config["margin"]]
        stitching_methods = ["exact-clipping"]
    for padding in padding_list:
        for img_pixels_detection in tile_size_list:
            for margin in margin_list:
                if margin < 1:
                    margin = int(margin * img_pixels_detection)
                if img_pixels_detection <= 2 * margin:
                    continue
                tmp_config = config.copy()
                tmp_config["margin"] = margin
                tmp_config["img_pixels_detection"] = img_pixels_detection
                for stride in get_stride(tmp_config):
                    for stitch in stitching_methods:
                        combi.append({"img_pixels_detection": img_pixels_detection, "margin": margin, "padding": padding,
                                      "stitching": stitch, "stride": stride})
    return combi


def method_name(combi: dict) -> str:
    """main.py:302"""
    return (f"size={combi['img_pixels_detection']}_stride={combi['stride']}_margin={combi['margin']}"
            f"_padding={combi['padding']}_stitching={combi['stitching']}")


def cheb_weight_table(patch_size: int):
    """patch_weights(S, 0.5, 'exp') by Chebyshev distance d = 0 .. S // 2 to the patch centre, float32: the table
    flair_detect_blend_accum reads for 'average_weights'."""
    import numpy as np
    w = patch_weights(patch_size, sigma=0.5, mode="exp")
    c = patch_size // 2
    return np.ascontiguousarray(w[c - np.arange(c + 1), c], dtype=np.float32)


class OverlapStitch:
    """Device state of one overlap-stitched job ('average', 'average_weights' or 'max') over the windows of ``grid``
    (tile_grid rows, job order): ``add`` the model's output for job windows [b0, b0 + B) in order, then ``finish``.

    'average' / 'average_weights' accumulate sum(w p) and sum(w) in a ring of K = S - 2m raster columns (x mod K): the job
    runs columns outer, so once the windows of one column are in, every pixel left of the next column's core is final and
    is flushed to the output before that column's first window.  A batch that straddles a column boundary is split into one
    launch per column.  'max' keeps its running (class, probability) in the output itself."""

    def __init__(self, method: str, grid, patch_size: int, margin: int, n_classes: int, raster_h: int, raster_w: int, device):
        import numpy as np
        if method not in STITCHING[1:]:
            raise ValueError(f"no overlap stitching named {method!r}")
        self.method, self.S, self.m, self.C = method, int(patch_size), int(margin), int(n_classes)
        self.H, self.W, self.K = int(raster_h), int(raster_w), self.S - 2 * self.m
        self.grid = np.asarray(grid)
        self.out = torch.zeros(2, self.H, self.W, dtype=torch.float32, device=device)
        self.ring = None if method == "max" else torch.zeros(self.C + 1, self.H, self.K, dtype=torch.float32, device=device)
        self.wtab = (torch.from_numpy(cheb_weight_table(self.S)).to(device) if method == "average_weights" else None)
        xs = self.grid[:, 0]
        self._col_start = np.concatenate([[True], xs[1:] != xs[:-1]])
        self._flushed = 0   # raster columns [0, _flushed) are final in self.out

    def _flush(self, hi: int):
        lo = self._flushed
        if hi > lo:
            # columns past lo + K lie between two columns' cores (stride > K): no window reached them, nothing to flush
            L.check(L.lib().flair_detect_blend_flush(L.ptr(self.ring), self.C, self.K, lo, min(hi, lo + self.K), L.ptr(self.out),
                                                     self.H, self.W, L.stream()), "flair_detect_blend_flush")
            self._flushed = hi

    def add(self, b0: int, tiles: torch.Tensor, logits: torch.Tensor = None, preds: torch.Tensor = None, prob: torch.Tensor = None,
            logits_q: torch.Tensor = None):
        """tiles: the device rows of job windows [b0, b0 + B); logits fp32 (B, C, S, S), or logits_q fp32 (B, C, S/4, S/4)
        (resized x4 per pixel in the kernel), or (preds u8, prob f32) (B, S, S) from predict_classes (method 'max' only)."""
        B = tiles.shape[0]
        q4 = "_q4" if logits_q is not None else ""
        if q4:
            if logits is not None or preds is not None:
                raise ValueError("logits_q excludes logits and preds")
            if self.S % 4 or tuple(logits_q.shape[2:]) != (self.S // 4, self.S // 4):
                raise ValueError(f"logits_q must be (B, C, {self.S} / 4, {self.S} / 4) with a patch size divisible by 4")
            logits = logits_q
        cuts = [b0] + [b for b in range(b0 + 1, b0 + B) if self._col_start[b]] + [b0 + B]
        for s, e in zip(cuts[:-1], cuts[1:]):
            x0 = int(self.grid[s, 0])
            ys = self.grid[s:e, 1]
            x_lo, x_hi = max(x0 + self.m, 0), min(x0 + self.S - self.m, self.W)
            y_lo, y_hi = max(int(ys.min()) + self.m, 0), min(int(ys.max()) + self.S - self.m, self.H)
            t = tiles[s - b0:e - b0]
            if self.method == "max":
                if preds is not None:
                    rc = L.lib().flair_detect_stitch_max_preds(L.ptr(preds[s - b0:e - b0]), L.ptr(prob[s - b0:e - b0]), e - s, self.S,
                                                               self.m, L.ptr(t), x_lo, x_hi, y_lo, y_hi, L.ptr(self.out), self.H, self.W,
                                                               L.stream())
                    L.check(rc, "flair_detect_stitch_max_preds")
                else:
                    fn = "flair_detect_stitch_max" + q4
                    rc = getattr(L.lib(), fn)(L.ptr(logits[s - b0:e - b0]), e - s, self.C, self.S, self.m, L.ptr(t),
                                              x_lo, x_hi, y_lo, y_hi, L.ptr(self.out), self.H, self.W, L.stream())
                    L.check(rc, fn)
                continue
            if self._col_start[s]:
                self._flush(min(x0 + self.m, self.W))
            fn = "flair_detect_blend_accum" + q4
            rc = getattr(L.lib(), fn)(L.ptr(logits[s - b0:e - b0]), e - s, self.C, self.S, self.m, L.ptr(t),
                                      L.ptr(self.wtab), x_lo, x_hi, y_lo, y_hi, L.ptr(self.ring), self.H, self.W, L.stream())
            L.check(rc, fn)

    def finish(self) -> torch.Tensor:
        if self.ring is not None:
            self._flush(self.W)
        return self.out


class ZoneDetector:
    """``model`` over a whole raster: windows are cut, normalised, inferred, converted and stitched on the device; the
    raster goes up once as stored bytes and the result comes down once.

    A config with a ``stitching`` key is one combination of the comparison grid (main.py:287-298, ``gen_param_combination``)
    and must carry ``stride``; without one the pipeline is the default (exact clipping, stride ``get_stride``)."""

    def __init__(self, model, config: dict):
        import ctypes as C
        self.model = model
        self.S = int(config["img_pixels_detection"])
        self.margin = int(config["margin"])
        self.output_type = config["output_type"]
        if self.output_type not in OUTPUT_TYPES:
            raise ValueError("The output type has not been interpreted.")
        self.stitching = config.get("stitching")
        if self.stitching is None:
            if config.get("overlap_strat"):
                raise NotImplementedError("overlap_strat describes a comparison grid: expand it with gen_param_combination(config) "
                                          "and run one ZoneDetector per combination (or compare())")
            self.stitching = "exact-clipping"
            self.stride = get_stride(config)[0]
        else:
            if self.stitching not in STITCHING:
                raise ValueError(f"unknown stitching {self.stitching!r} (one of {', '.join(STITCHING)})")
            if config.get("stride") is None:
                raise ValueError("a stitching combination needs its 'stride' (gen_param_combination)")
            if config.get("padding", "no-padding") != "no-padding":
                raise ValueError(f"padding {config['padding']!r} is not implemented (only 'no-padding')")
            self.stride = int(config["stride"])
            if self.stride < 1:
                raise ValueError("stride must be a positive number of pixels")
        # class_prob output is stitched by exact clipping whatever the method (compare.py:67-68)
        self.blend = None if self.stitching == "exact-clipping" or self.output_type == "class_prob" else self.stitching
        self.batch_size = int(config.get("batch_size", 4))
        self.channels = [int(c) for c in config["channels"]]
        norma = config["norma_task"][0]
        self.norm_type = norma["norm_type"] if norma["norm_type"] in ("custom", "scaling") else "scaling"
        means, stds = norma.get("norm_means", []), norma.get("norm_stds", [])
        if self.norm_type == "custom" and len(means) != len(stds):
            self.norm_type = "scaling"  # dataset.py:77-81
        n = len(self.channels)
        self._ch = (C.c_int * n)(*self.channels)
        self._means = (C.c_double * n)(*[float(m) for m in means[:n]]) if self.norm_type == "custom" else None
        self._stds = (C.c_double * n)(*[float(s) for s in stds[:n]]) if self.norm_type == "custom" else None
        self.n_classes = int(config["n_classes"])
        self.classes = config.get("classes")
        # quarter-resolution logits straight into the _q4 kernels (no x4 pass, no tile-sized logits); FLAIR_ZD_QUARTER=0: the x4 path
        want = os.environ.get("FLAIR_ZD_QUARTER", "1" if QUARTER_DEFAULT else "0") != "0"
        self.quarter = want and hasattr(model, "forward_quarter") and self.S % 4 == 0
        # test-time augmentation (flair_amd.tta): every batch of windows becomes a (class, mean probability) pair, which
        # the _preds kernels stitch whatever the model
        self.tta = tta_codes(config.get("tta"))
        if self.tta is not None:
            if self.output_type != "argmax":
                raise ValueError("tta needs output_type 'argmax': 'class_prob' writes every class's probability, and the ensemble keeps "
                                 "only the winner's")
            if self.blend not in (None, "max"):
                raise ValueError(f"tta with stitching {self.stitching!r} is not implemented: 'average' and 'average_weights' blend "
                                 "per-class probabilities, and the ensemble keeps only the winner's (use 'exact-clipping' or 'max')")
        self.window_confmats = None   # run(raster, truth): (n, C, C) int64 on the device, one per window in job order
        self.window_rects = None      # and their (col_off, row_off, width, height) core rectangles, numpy int32 (n, 4)

    def _check_truth(self, truth_u8: torch.Tensor, Hr: int, Wr: int):
        if not truth_u8.is_cuda or truth_u8.dtype != torch.uint8 or tuple(truth_u8.shape) != (Hr, Wr):
            raise ValueError(f"truth must be a ({Hr}, {Wr}) uint8 tensor on the HIP device, the raster's extent "
                             f"(got {tuple(truth_u8.shape)} {truth_u8.dtype} on {truth_u8.device})")
        if self.output_type != "argmax":
            raise ValueError("metrics need the 'argmax' output: band 0 of 'class_prob' is a probability, not a class")
        if not self.classes:
            raise ValueError("metrics need config['classes'] (the class weights and names of the confusion matrix)")
        model_c = getattr(self.model, "classes", None) or getattr(self.model, "num_labels", None) or self.n_classes
        if int(model_c) != len(self.classes) or self.n_classes != len(self.classes):
            raise ValueError(f"the model has {model_c} classes (config n_classes {self.n_classes}), config['classes'] lists "
                             f"{len(self.classes)}")

    def _fast_preds(self, mode: int) -> bool:
        """'argmax' output from a U-Net in eval mode: class and probability leave the head convolution's epilogue, the logits
        are never written"""
        if not (mode == 0 and hasattr(self.model, "predict_classes") and not self.model.training):
            return False
        if getattr(self.model, "classes", self.n_classes) != self.n_classes:
            raise RuntimeError(f"model has {self.model.classes} classes, config says {self.n_classes}")
        return True

    def _tta_preds(self, imgs: torch.Tensor):
        """(class u8, mean probability f32), both (B, S, S), of the ensemble over ``self.tta`` for a batch of gathered windows"""
        if self._fast_preds(0):
            return self.model.predict_classes(imgs, want_prob=True, tta=self.tta)
        if self.quarter:
            return tta_predict(self._logits_quarter, imgs, self.tta, want_prob=True, quarter=True)
        return tta_predict(self._logits, imgs, self.tta, want_prob=True)

    def _logits(self, imgs: torch.Tensor) -> torch.Tensor:
        if hasattr(self.model, "forward_full"):
            # HuggingFace provider (SegFormer): `.logits` come at 1/4 of the tile size, which neither the margin crop nor
            # convert (compare.py:69-82) rescale; the x4 bilinear upsample (align_corners=False) the library itself applies
            # in front of its loss brings them to tile resolution first
            logits = self.model.forward_full(imgs)
        else:
            logits = self.model(imgs).float().contiguous()
        if logits.shape[1] != self.n_classes:
            raise RuntimeError(f"model returned {logits.shape[1]} classes, config says {self.n_classes}")
        return logits

    def _logits_quarter(self, imgs: torch.Tensor) -> torch.Tensor:
        logits = self.model.forward_quarter(imgs)
        if logits.shape[1] != self.n_classes or tuple(logits.shape[2:]) != (self.S // 4, self.S // 4) or logits.dtype != torch.float32:
            raise RuntimeError(f"forward_quarter returned {tuple(logits.shape)} {logits.dtype}, expected fp32 "
                               f"(B, {self.n_classes}, {self.S // 4}, {self.S // 4})")
        return logits.contiguous()

    @torch.no_grad()
    def run(self, raster_u8: torch.Tensor, truth_u8: torch.Tensor = None) -> torch.Tensor:
        """The output raster.  With ``truth_u8`` ((H, W) uint8 label raster on the device) the run also leaves
        ``window_confmats`` / ``window_rects``: each window's confusion matrix over its margin-cropped core against
        truth - 1, from the window's own prediction (exact clipping) or from the finished raster (overlap methods)."""
        if not raster_u8.is_cuda or raster_u8.dtype != torch.uint8 or raster_u8.dim() != 3:
            raise RuntimeError("raster must be a (bands, H, W) uint8 tensor on the HIP device")
        raster_u8 = raster_u8.contiguous()
        bands, Hr, Wr = raster_u8.shape
        dev = raster_u8.device
        grid_np = tile_grid((Wr, Hr), self.S, self.margin, self.stride)
        grid = torch.from_numpy(grid_np).to(dev)
        confmats, self.window_confmats, self.window_rects = None, None, None
        if truth_u8 is not None:
            self._check_truth(truth_u8, Hr, Wr)
            truth_u8 = truth_u8.contiguous()
            C = self.n_classes
            confmats = torch.zeros(len(grid_np), C, C, dtype=torch.int64, device=dev)
            K = self.S - 2 * self.margin
            self.window_rects = np.stack([grid_np[:, 0] + self.margin, grid_np[:, 1] + self.margin, np.full(len(grid_np), K),
                                          np.full(len(grid_np), K)], axis=1).astype(np.int32)
        mode = OUTPUT_TYPES[self.output_type]
        blend = (OverlapStitch(self.blend, grid_np, self.S, self.margin, self.n_classes, Hr, Wr, dev) if self.blend else None)
        if blend is not None:
            out = blend.out
        else:
            out = (torch.zeros(2, Hr, Wr, dtype=torch.float32, device=dev) if mode == 0
                   else torch.zeros(self.n_classes, Hr, Wr, dtype=torch.uint8, device=dev))
        from .data_feed import NORM_CODES
        for b0 in range(0, grid.shape[0], self.batch_size):
            tiles = grid[b0:b0 + self.batch_size].contiguous()
            B = tiles.shape[0]
            imgs = torch.empty(B, len(self.channels), self.S, self.S, dtype=torch.float32, device=dev)
            L.check(L.lib().flair_gather_tiles(L.ptr(raster_u8), bands, Hr, Wr, L.ptr(tiles), B, self.S, self._ch,
                                               len(self.channels), NORM_CODES[self.norm_type], self._means, self._stds,
                                               L.ptr(imgs), L.stream()), "flair_gather_tiles")
            if blend is not None:
                if self.tta is not None:
                    preds, prob = self._tta_preds(imgs)
                    blend.add(b0, tiles, preds=preds, prob=prob)
                elif self.blend == "max" and self._fast_preds(mode):
                    preds, prob = self.model.predict_classes(imgs, want_prob=True)
                    blend.add(b0, tiles, preds=preds, prob=prob)
                elif self.quarter:
                    blend.add(b0, tiles, logits_q=self._logits_quarter(imgs))
                else:
                    blend.add(b0, tiles, logits=self._logits(imgs))
                continue
            if self.tta is not None or self._fast_preds(mode):
                preds, prob = self._tta_preds(imgs) if self.tta is not None else self.model.predict_classes(imgs, want_prob=True)
                L.check(L.lib().flair_detect_stitch_preds(L.ptr(preds), L.ptr(prob), B, self.S, self.margin, L.ptr(tiles), L.ptr(out),
                                                          Hr, Wr, L.stream()), "flair_detect_stitch_preds")
                if confmats is not None:
                    L.check(L.lib().flair_zone_window_confmat_preds(L.ptr(preds), B, self.n_classes, self.S, self.margin, L.ptr(tiles),
                                                                    L.ptr(truth_u8), Hr, Wr, L.ptr(confmats[b0:b0 + B]), L.stream()),
                            "flair_zone_window_confmat_preds")
                continue
            logits, q4 = (self._logits_quarter(imgs), "_q4") if self.quarter else (self._logits(imgs), "")
            L.check(getattr(L.lib(), "flair_detect_stitch" + q4)(L.ptr(logits), B, self.n_classes, self.S, self.margin, mode, L.ptr(tiles),
                                                                 L.ptr(out), Hr, Wr, L.stream()), "flair_detect_stitch" + q4)
            if confmats is not None:
                fn = "flair_zone_window_confmat_logits" + q4
                L.check(getattr(L.lib(), fn)(L.ptr(logits), B, self.n_classes, self.S, self.margin, L.ptr(tiles), L.ptr(truth_u8), Hr, Wr,
                                             L.ptr(confmats[b0:b0 + B]), L.stream()), fn)
        if blend is not None:
            out = blend.finish()
            if confmats is not None:   # an overlap method's window is scored on the finished raster
                for b0 in range(0, len(grid_np), _MAX_GRID_Y):
                    B = min(_MAX_GRID_Y, len(grid_np) - b0)
                    L.check(L.lib().flair_zone_window_confmat_raster(L.ptr(out), B, self.n_classes, self.S, self.margin,
                                                                     L.ptr(grid[b0:b0 + B]), L.ptr(truth_u8), Hr, Wr,
                                                                     L.ptr(confmats[b0:b0 + B]), L.stream()),
                            "flair_zone_window_confmat_raster")
        self.window_confmats = confmats
        return out

    def write(self, out: torch.Tensor, path, source=None, **kw) -> dict:
        """What ``run`` returned, as the file the reference's pipeline ends in (main.py:206-232, :386-428): one tiled LZW BigTIFF with
        tiles of ``img_pixels_detection``, encoded on the device (raster_writer.write_raster, which takes ``kw``: interleave, bigtiff,
        group_bytes, tile).  'argmax': band 1 the class, band 2 the confidence as uint8(p * 255); 'class_prob': the
        ``n_classes`` probability bytes.  ``source``: the input raster's file, whose GeoTIFF tags the output takes over."""
        from . import raster_writer
        bands, dtype = (2, torch.float32) if self.output_type == "argmax" else (self.n_classes, torch.uint8)
        if not torch.is_tensor(out) or out.dim() != 3 or out.shape[0] != bands or out.dtype != dtype:
            raise ValueError(f"output_type {self.output_type!r} writes a ({bands}, H, W) {dtype} raster, the one run returns")
        kw.setdefault("tile", self.S)
        if source is not None:
            kw.setdefault("geo_tags", raster_writer.read_geo_tags(source))
        return raster_writer.write_raster(path, out, scale=(1.0, 255.0) if self.output_type == "argmax" else None, **kw)

    def run_to_file(self, raster_u8: torch.Tensor, path, truth_u8: torch.Tensor = None, source=None, **kw) -> torch.Tensor:
        """``run`` followed by ``write``; returns the raster ``run`` returned"""
        out = self.run(raster_u8, truth_u8)
        self.write(out, path, source=source, **kw)
        return out

    def read(self, path, device=None) -> torch.Tensor:
        """The (bands, H, W) uint8 raster of the file ``input_img_path`` names, decoded on the device (raster_reader.read_raster); a
        file with fewer bands than ``channels`` asks for (band numbers from 1, as rasterio counts them) is refused here."""
        from . import raster_reader
        raster = raster_reader.read_raster(path, torch.device("cuda", torch.cuda.current_device()) if device is None else device)
        if raster.shape[0] < max(self.channels):
            raise ValueError(f"{os.fspath(path)!r} has {raster.shape[0]} bands, config['channels'] asks for band {max(self.channels)}")
        return raster

    def run_files(self, src, dst, truth=None, **kw) -> torch.Tensor:
        """From a file to a file: ``read(src)``, ``run``, ``write(dst, source=src)`` (``kw`` goes to ``write``).  ``truth``: a label raster
        file of the same extent, whose first band is ``run``'s ``truth_u8``.  Returns the raster ``run`` returned."""
        from . import raster_reader
        raster = self.read(src)
        truth_u8 = None if truth is None else raster_reader.read_raster(truth, raster.device)[0]
        return self.run_to_file(raster, dst, truth_u8, source=src, **kw)


def compare(model, config: dict, raster_u8: torch.Tensor) -> dict:
    """The comparison loop of main.py:275-372 without raster files or metrics: one ZoneDetector per combination of
    ``gen_param_combination(config)``.  Returns {method name (main.py:302): (output raster, wall ms of the synchronised run)}."""
    import time
    results = {}
    for combi in gen_param_combination(config):
        cfg = dict(config)
        cfg.update(combi)
        det = ZoneDetector(model, cfg)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = det.run(raster_u8)
        torch.cuda.synchronize()
        results[method_name(combi)] = (out, (time.perf_counter() - t0) * 1e3)
    return results


# ------------------------------------------------------------------------------------------------------------------
# Tile bookkeeping of the overlap strategies (src/zone_detect/test/tiles.py, test/pixel_operation.py): host integer /
# float64 arithmetic on small maps, mirrored for callers that schedule overlapping windows themselves.  Pinned by
# tests/golden/tiling_reference.json (the reference functions, imported directly).

def out_of_bounds(bigbox, box):
    """tiles.py:17-27 — per coordinate of ``box``: is it outside ANY of the four bounds of ``bigbox``
    (left, right, bottom, top), compared as the reference does (every coordinate against all four)."""
    left, right, bottom, top = bigbox
    return [bool(c < left or c > right or c < bottom or c > top) for c in box]


def get_tile_coord(start: int, end: int, limit: int, patch_size: int, stride: int):
    """tiles.py:30-51 — tile origins along one axis that intersect [start, end): multiples of ``stride`` below ``end``,
    the ones that would pass ``limit`` pulled back to limit - patch_size (ascending; the reference's order is a set's)."""
    last = limit - patch_size
    if last < 0:
        return []
    origins = {min(i, last) if i + patch_size > limit else i for i in range(0, end, stride)}
    return sorted(o for o in origins if o + patch_size > start and o < end)


def _axis_cover(lo: int, hi: int, limit: int, patch_size: int, stride: int):
    """how many tiles of one axis cover each position of [lo, hi)"""
    import numpy as np
    n = np.zeros(hi - lo, dtype=np.int64)
    for o in get_tile_coord(lo, hi, limit, patch_size, stride):
        a, b = max(o, lo), min(o + patch_size, hi)
        if b > a:
            n[a - lo:b - lo] += 1
    return n


def patch_overlap(image_size, patch_size: int, query_bounds, stride: int):
    """tiles.py:54-94 — number of tiles covering every pixel of the query rectangle (x_min, x_max, y_min, y_max); the
    tiles form a grid, so the count is the outer product of the per-axis coverages."""
    import numpy as np
    x_min, x_max, y_min, y_max = query_bounds
    cx = _axis_cover(x_min, x_max, image_size[0], patch_size, stride)
    cy = _axis_cover(y_min, y_max, image_size[1], patch_size, stride)
    return np.outer(cy, cx).astype(np.uint8)


def patch_weights(patch_size: int, sigma: float, mode: str):
    """tiles.py:97-108 — weight of a pixel by its Chebyshev distance d to the patch centre:
    'gaussian': exp(-d / d_max^2) / (2 sigma^2); anything else: exp(-d / d_max * sigma)."""
    import numpy as np
    c = patch_size // 2
    ax = np.abs(np.arange(patch_size) - c)
    dist = np.maximum(ax[:, None], ax[None, :])
    if mode == "gaussian":
        return np.exp(-dist / dist.max() ** 2) / (2 * sigma ** 2)
    return np.exp(-dist / dist.max() * sigma)


def total_weights(image_size, patch_size: int, query_bounds, stride: int, track_steps: bool = False):
    """tiles.py:111-168 — sum over the tiles intersecting the query of their 'exp' patch weights (sigma 0.5), float32."""
    import numpy as np
    x_min, x_max, y_min, y_max = query_bounds
    acc = np.zeros((y_max - y_min, x_max - x_min), dtype=np.float32)
    w = patch_weights(patch_size, sigma=0.5, mode="exp")
    steps = []
    for ty in get_tile_coord(y_min, y_max, image_size[1], patch_size, stride):
        ya, yb = max(ty, y_min), min(ty + patch_size, y_max)
        for tx in get_tile_coord(x_min, x_max, image_size[0], patch_size, stride):
            xa, xb = max(tx, x_min), min(tx + patch_size, x_max)
            if yb > ya and xb > xa:
                acc[ya - y_min:yb - y_min, xa - x_min:xb - x_min] += w[ya - ty:yb - ty, xa - tx:xb - tx]
                if track_steps:
                    steps.append(acc.copy())
    return acc, steps


def slice_pixels(img_size, patch_size: int, margin: int, stride: int):
    """pixel_operation.py:1-60 — margin-cropped boxes (x_min, x_max, y_min, y_max) of a regular grid with step
    ``stride``, plus a last row / column / corner flush with the image edge when the grid does not end there."""
    x_size, y_size = img_size
    k = patch_size - 2 * margin

    def axis(size):
        starts = [o for o in range(0, size + 1, stride) if o + k <= size]
        if size - k > 0 and (size - k) % stride != 0:
            starts.append(size - k)
        return starts

    xs, ys = axis(x_size), axis(y_size)
    return sorted({(x, x + k, y, y + k) for y in ys for x in xs})
