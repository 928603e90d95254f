"""zone_detect's overlap stitching on the device ('average', 'average_weights', 'max'; csrc/zone_stitch.hip through
flair_detect_blend_accum / _flush, flair_detect_stitch_max(_preds)) against the float64 restatement of
tests/test_zone_stitch_cpu.py.  Class band: exact wherever the restatement's decision gap exceeds parity.GAP; probability
band within 1e-5 for identical logits.  Bit-exact: batch-split invariance, and the reduction to exact clipping wherever every
pixel has one window."""
import importlib.util
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("zone_stitch_restatement", os.path.join(os.path.dirname(__file__), "test_zone_stitch_cpu.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

MEANS = [105.08, 110.87, 101.82, 106.38, 53.26]
STDS = [52.17, 45.38, 44, 39.69, 79.3]
METHODS = ("average", "average_weights", "max")


def _stitch_dev(dev, method, logits, grid, H, W, S, m, batch):
    """OverlapStitch over precomputed logits (N, C, S, S) fed ``batch`` windows at a time."""
    from flair_amd.zone_detect import OverlapStitch
    st = OverlapStitch(method, grid, S, m, logits.shape[1], H, W, dev)
    tiles_all = torch.from_numpy(grid).to(dev)
    lg = torch.from_numpy(np.ascontiguousarray(logits)).to(dev)
    for b0 in range(0, len(grid), batch):
        st.add(b0, tiles_all[b0:b0 + batch].contiguous(), logits=lg[b0:b0 + batch].contiguous())
    return st.finish().cpu().numpy()


def _exact_dev(dev, logits, grid, H, W, S, m):
    from flair_amd import _lib as L
    out = torch.zeros(2, H, W, device=dev)
    lg = torch.from_numpy(np.ascontiguousarray(logits)).to(dev)
    t = torch.from_numpy(grid).to(dev)
    L.check(L.lib().flair_detect_stitch(L.ptr(lg), lg.shape[0], lg.shape[1], S, m, 0, L.ptr(t), L.ptr(out), H, W, L.stream()))
    return out.cpu().numpy()


def _check(name, got, want, gap, prob_tol=1e-5):
    from oracle import parity
    assert got.shape == want.shape and got.dtype == np.float32
    unc = np.isinf(gap)
    assert (got[:, unc] == 0).all(), f"{name}: a pixel no window reached was written"
    cov = ~unc
    parity.assert_mask_parity(name, want[0][cov], got[0][cov], gap[cov])
    assert np.abs(got[1][cov] - want[1][cov]).max() < prob_tol, (name, np.abs(got[1][cov] - want[1][cov]).max())


@pytest.mark.parametrize("C", [13, 19])
@pytest.mark.parametrize("m,stride", [(0, 16), (0, 24), (0, 64), (8, 16), (8, 24), (8, 48), (8, 56)])
def test_overlap_modes_vs_restatement(dev, m, stride, C):
    """150 x 190 raster (no multiple of any stride), S = 64; stride 56 > K = 48 leaves uncovered bands at zero."""
    from flair_amd.zone_detect import tile_grid
    S, H, W = 64, 150, 190
    grid = tile_grid((W, H), S, m, stride)
    lg = np.random.default_rng(100 * m + stride + C).normal(0, 3, size=(len(grid), C, S, S)).astype(np.float32)
    for method in METHODS:
        want, gap = R.stitch_np(lg, grid, H, W, S, m, method)
        got = _stitch_dev(dev, method, lg, grid, H, W, S, m, batch=5)
        _check(f"zone_stitch_{method}_m{m}_s{stride}_C{C}", got, want, gap)


def test_batch_split_invariance_bit_exact(dev):
    from flair_amd.zone_detect import tile_grid
    S, m, H, W, C = 64, 8, 150, 190, 13
    grid = tile_grid((W, H), S, m, 16)
    lg = np.random.default_rng(7).normal(0, 3, size=(len(grid), C, S, S)).astype(np.float32)
    for method in METHODS:
        ref = _stitch_dev(dev, method, lg, grid, H, W, S, m, batch=1)
        for b in (3, 7, 1):
            got = _stitch_dev(dev, method, lg, grid, H, W, S, m, batch=b)
            assert np.array_equal(got, ref), (method, b)


def test_stride_k_reduces_to_exact_clipping_bit_exact(dev):
    """Raster a multiple of K: every pixel has one window, so 'average' and 'max' are today's exact clipping, bit for bit."""
    from flair_amd.zone_detect import tile_grid
    S, m, C = 64, 8, 19
    K = S - 2 * m
    H, W = 3 * K, 4 * K
    grid = tile_grid((W, H), S, m, K)
    lg = np.random.default_rng(3).normal(0, 3, size=(len(grid), C, S, S)).astype(np.float32)
    want = _exact_dev(dev, lg, grid, H, W, S, m)
    for method in ("average", "max"):
        assert np.array_equal(_stitch_dev(dev, method, lg, grid, H, W, S, m, batch=3), want), method


def test_abi_rejects_bad_arguments(dev):
    from flair_amd import _lib as L
    lg = torch.zeros(1, 33, 16, 16, device=dev)
    t = torch.zeros(1, 6, dtype=torch.int32, device=dev)
    ring = torch.zeros(34, 16, 16, device=dev)
    out = torch.zeros(2, 16, 16, device=dev)
    lib = L.lib()
    assert lib.flair_detect_blend_accum(L.ptr(lg), 1, 33, 16, 0, L.ptr(t), None, 0, 16, 0, 16, L.ptr(ring), 16, 16, L.stream()) == -2
    assert lib.flair_detect_blend_accum(L.ptr(lg), 1, 13, 16, 2, L.ptr(t), None, 0, 13, 0, 16, L.ptr(ring), 16, 16, L.stream()) == -2
    assert lib.flair_detect_blend_accum(L.ptr(lg), 1, 13, 16, 0, L.ptr(t), None, 0, 16, 0, 17, L.ptr(ring), 16, 16, L.stream()) == -2
    assert lib.flair_detect_blend_flush(L.ptr(ring), 13, 8, 0, 9, L.ptr(out), 16, 16, L.stream()) == -2
    assert lib.flair_detect_stitch_max(L.ptr(lg), 1, 0, 16, 0, L.ptr(t), 0, 16, 0, 16, L.ptr(out), 16, 16, L.stream()) == -2
    assert lib.flair_detect_stitch_max_preds(None, None, 1, 16, 0, L.ptr(t), 0, 16, 0, 16, L.ptr(out), 16, 16, L.stream()) == -1
    assert lib.flair_detect_stitch_max(L.ptr(lg), 1, 13, 16, 9, L.ptr(t), 0, 16, 0, 16, L.ptr(out), 16, 16, L.stream()) == -2


# ---------------------------------------------------------------------------------------------- ZoneDetector

class _Stub:
    """logits = a fixed (C, S, S) bias + a 1 x 1 mix of the input: they depend on the pixel's place in the window, so
    overlapping windows disagree."""

    training = False

    def __init__(self, C, S, bands, seed=0):
        g = np.random.default_rng(seed)
        self.bias = g.normal(0, 2, size=(C, S, S)).astype(np.float32)
        self.mix = g.normal(0, 0.7, size=(C, bands)).astype(np.float32)
        self._dev = {}

    def __call__(self, x):
        if x.device not in self._dev:
            self._dev[x.device] = (torch.from_numpy(self.bias).to(x.device), torch.from_numpy(self.mix).to(x.device))
        b, w = self._dev[x.device]
        return torch.einsum("bkhw,ck->bchw", x, w) + b

    def logits_np(self, x):   # float64
        return np.einsum("bkhw,ck->bchw", x.astype(np.float64), self.mix.astype(np.float64)) + self.bias


def _windows_np(raster, cfg, grid):
    """dataset.py:90-113 in image coordinates: boundless read (0 outside), band selection, normalisation."""
    from oracle import data_feed
    S = cfg["img_pixels_detection"]
    _, H, W = raster.shape
    norma = cfg["norma_task"][0]
    out = []
    for x0, y0 in grid[:, :2]:
        w = np.zeros((len(cfg["channels"]), S, S), raster.dtype)
        ya, yb, xa, xb = max(y0, 0), min(y0 + S, H), max(x0, 0), min(x0 + S, W)
        w[:, ya - y0:yb - y0, xa - x0:xb - x0] = raster[[c - 1 for c in cfg["channels"]], ya:yb, xa:xb]
        out.append(data_feed.norm_np(w, norma["norm_type"], norma.get("norm_means", []), norma.get("norm_stds", [])))
    return np.stack(out)


def _zcfg(C, **kw):
    c = {"img_pixels_detection": 64, "margin": 8, "output_type": "argmax", "n_classes": C, "batch_size": 5,
         "channels": [1, 2, 3, 4, 5], "norma_task": [{"norm_type": "custom", "norm_means": MEANS, "norm_stds": STDS}]}
    c.update(kw)
    return c


def test_zone_detector_stub_model_every_mode(dev):
    from flair_amd.zone_detect import ZoneDetector, tile_grid
    C, S, m, stride = 13, 64, 8, 24
    raster = np.random.default_rng(21).integers(0, 256, size=(5, 150, 190), dtype=np.uint8)
    H, W = raster.shape[1:]
    stub = _Stub(C, S, 5)
    grid = tile_grid((W, H), S, m, stride)
    lg = stub.logits_np(_windows_np(raster, _zcfg(C), grid))
    r = torch.from_numpy(raster).to(dev)
    for method in METHODS:
        want, gap = R.stitch_np(lg, grid, H, W, S, m, method)
        got = ZoneDetector(stub, _zcfg(C, stitching=method, stride=stride, padding="no-padding")).run(r).cpu().numpy()
        # the stub's logits on the device are fp32 (einsum over 5 bands), the restatement's fp64
        _check(f"zone_detector_stub_{method}", got, want, gap, prob_tol=5e-5)
    got = ZoneDetector(stub, _zcfg(C, stitching="exact-clipping", stride=stride)).run(r).cpu().numpy()
    gap = np.zeros((H, W))
    want = R.exact_np(lg, grid, H, W, S, m, gap_out=gap)
    _check("zone_detector_stub_exact_clipping_stride24", got, want, gap, prob_tol=5e-5)
    # class_prob: exact clipping with the combination's stride, whatever the method (compare.py:67-68)
    ref = ZoneDetector(stub, _zcfg(C, output_type="class_prob", stitching="exact-clipping", stride=stride)).run(r)
    assert ref.dtype == torch.uint8 and ref.shape == (C, H, W)
    for method in METHODS:
        got = ZoneDetector(stub, _zcfg(C, output_type="class_prob", stitching=method, stride=stride)).run(r)
        assert torch.equal(got, ref), method
    with pytest.raises(NotImplementedError):
        ZoneDetector(stub, _zcfg(C, overlap_strat=True, strategies={"tiling": {"stride_range": [0.5]}}))
    with pytest.raises(ValueError):
        ZoneDetector(stub, _zcfg(C, stitching="average", stride=stride, padding="mirror"))


def test_accumulator_memory_is_a_column_ring(dev):
    """5 x 1024 x 3000, C = 19, S = 64, m = 8, stride 16: a full-raster accumulator would be 20 x 1024 x 3000 x 4 = 245 MB;
    the ring is 20 x 1024 x 48 x 4 = 3.9 MB."""
    from flair_amd.zone_detect import ZoneDetector
    C, S, m, B = 19, 64, 8, 16
    H, W = 1024, 3000
    raster = torch.randint(0, 256, (5, H, W), dtype=torch.uint8, device=dev)
    stub = _Stub(C, S, 5)
    det = ZoneDetector(stub, _zcfg(C, stitching="average_weights", stride=16, batch_size=B))
    det.run(raster[:, :128, :128].contiguous())   # stub weights on the device
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    start = torch.cuda.memory_allocated(dev)
    out = det.run(raster)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - start
    out_b, ring_b = 2 * H * W * 4, (C + 1) * H * (S - 2 * m) * 4
    batch_b = B * (5 + 3 * C) * S * S * 4     # images, the stub's einsum and its sum, the contiguous logits
    assert peak < out_b + ring_b + batch_b + (4 << 20), (peak, out_b, ring_b, batch_b)
    assert peak < 245e6 / 4
    assert (out[1] > 0).all()


def test_zone_detector_unet_vs_oracle(dev):
    """HIP U-Net (fp32, seeded oracle weights): 'average_weights' through logits, 'max' through predict_classes' (class,
    probability) maps; both against the oracle's logits run through the restatement, masks by the parity rule."""
    import flair_amd
    from flair_amd.zone_detect import ZoneDetector, tile_grid
    from oracle import unet_resnet34 as om
    C, S, m, stride = 19, 64, 8, 24
    ref = om.seeded_model(5, C, 6).eval()
    hip = flair_amd.create_model("unet", "resnet34", encoder_weights=None, in_channels=5, classes=C, compute_dtype="f32")
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip = hip.to(dev).eval()
    raster = np.random.default_rng(12).integers(0, 256, size=(5, 168, 200), dtype=np.uint8)
    H, W = raster.shape[1:]
    grid = tile_grid((W, H), S, m, stride)
    x = _windows_np(raster, _zcfg(C), grid)
    with torch.no_grad():
        lg = torch.cat([ref(torch.from_numpy(x[i:i + 16])) for i in range(0, len(x), 16)]).numpy()
    r = torch.from_numpy(raster).to(dev)
    for method in ("average_weights", "max"):
        want, gap = R.stitch_np(lg, grid, H, W, S, m, method)
        got = ZoneDetector(hip, _zcfg(C, stitching=method, stride=stride, batch_size=4)).run(r).cpu().numpy()
        _check(f"zone_detector_unet_{method}_168x200", got, want, gap, prob_tol=2e-3)


def test_zone_detector_segformer_average_vs_oracle(dev):
    import flair_amd
    from flair_amd.zone_detect import ZoneDetector, tile_grid
    from oracle import segformer as osf
    C, S, m, stride = 19, 128, 32, 40
    ref = osf.seeded_model(5, C, seed=2022, depths=[1, 1, 1, 1], decoder_hidden_size=256)
    hip = flair_amd.SegformerForSemanticSegmentation(num_channels=5, num_labels=C, compute_dtype="f32", depths=[1, 1, 1, 1],
                                                     decoder_hidden_size=256)
    hip.load_state_dict(ref.state_dict(), strict=True)
    hip = hip.to(dev).eval()
    raster = np.random.default_rng(4).integers(0, 256, size=(5, 200, 264), dtype=np.uint8)
    H, W = raster.shape[1:]
    cfg = _zcfg(C, img_pixels_detection=S, margin=m, stitching="average", stride=stride, batch_size=3)
    grid = tile_grid((W, H), S, m, stride)
    x = _windows_np(raster, cfg, grid)
    with torch.no_grad():
        lg = torch.cat([osf.logits(ref, torch.from_numpy(x[i:i + 8]))[1] for i in range(0, len(x), 8)]).numpy()
    want, gap = R.stitch_np(lg, grid, H, W, S, m, "average")
    got = ZoneDetector(hip, cfg).run(torch.from_numpy(raster).to(dev)).cpu().numpy()
    _check("zone_detector_segformer_average_200x264", got, want, gap, prob_tol=1e-4)


def test_compare_runs_every_combination(dev):
    from flair_amd.zone_detect import ZoneDetector, compare
    C = 13
    raster = torch.from_numpy(np.random.default_rng(5).integers(0, 256, size=(5, 150, 190), dtype=np.uint8)).to(dev)
    stub = _Stub(C, 64, 5, seed=3)
    cfg = _zcfg(C, overlap_strat=True, strategies={"tiling": {"stride_range": [0.25, 0.375]},
                                                   "stitching": {"enabled": True, "methods": ["average", "max"]}})
    t0 = time.perf_counter()
    res = compare(stub, cfg, raster)
    assert time.perf_counter() - t0 >= sum(ms for _, ms in res.values()) / 1e3
    names = [f"size=64_stride={s}_margin=8_padding=no-padding_stitching={meth}" for s in (16, 24) for meth in ("average", "max")]
    assert list(res) == names
    for name, (out, ms) in res.items():
        stride, meth = int(name.split("_stride=")[1].split("_")[0]), name.split("stitching=")[1]
        want = ZoneDetector(stub, _zcfg(C, stitching=meth, stride=stride, padding="no-padding")).run(raster)
        assert ms > 0 and torch.equal(out, want), name
